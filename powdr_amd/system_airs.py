"""The receive side of the execution bridge, the memory bus and the PC lookup: the three system AIRs that close a segment's buses
 — their constraint and interaction programs in the formats `prover.Prover` takes (the pattern of periphery.py; sends
+m, receives -m) — and the callers of the routines that make their traces on the device from the other AIRs' raw traces
(include/powdr_prover.h `pw_program_frequencies`, `pw_memory_boundary_trace`).

  program     preprocessed [pc, opcode, a .. g] (the bus-2 tuple of openvm_constraints.txt), main [freq]: row k is received freq times
  connector   2 rows, preprocessed [is_end] = (0, 1), main [pc, timestamp]: row 0 sends the initial state, row 1 receives the final one
  boundary    one row per touched location, sorted by (as, ptr): sends what the location held before its first access, receives what
              it holds after its last; `init*` / `fin*` are witness columns (from SOME initial memory to SOME final memory)

and the Poseidon2 compression chip (`pw_poseidon2_compress_trace`), the receive side of every hash a later AIR states:

  poseidon2   one permutation per row, 307 columns [mult, in[16], the cube and the seventh power of every S-box input, out[8]]:
              receives (left[8], right[8], out[8]) `mult` times on BUS_COMPRESS
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import abi, air_text, prover, stage
from .periphery import OP_PUSH_APC, OP_PUSH_CONST, _col, _join_tables, _neg_col, _tables

lib = abi.lib
lib.pw_program_frequencies.restype = C.c_int
lib.pw_program_frequencies.argtypes = [C.POINTER(prover.PwSegmentAir), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(prover.PwBusTuple)]
lib.pw_memory_boundary_trace.restype = C.c_int
lib.pw_memory_boundary_trace.argtypes = [C.POINTER(prover.PwSegmentAir), C.c_size_t, C.c_uint32, C.c_size_t, C.c_void_p, C.c_uint32,
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
lib.pw_poseidon2_compress_trace.restype = C.c_int
lib.pw_poseidon2_compress_trace.argtypes = [C.POINTER(prover.PwSegmentAir), C.c_size_t, C.c_uint32, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
lib.pw_system_traces_scratch_bytes.restype = C.c_size_t
lib.pw_system_traces_scratch_bytes.argtypes = []
lib.pw_system_traces_peak_bytes.restype = C.c_size_t
lib.pw_system_traces_peak_bytes.argtypes = []


class PwSystemTraceStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("table_slots", "occupied_slots", "tables", "walked", "additions", "lds_atomics", "global_atomics")]


lib.pw_system_traces_last_stats.restype = None
lib.pw_system_traces_last_stats.argtypes = [C.POINTER(PwSystemTraceStats)]
lib.pw_memory_boundary_set_start_slots.restype = C.c_int
lib.pw_memory_boundary_set_start_slots.argtypes = [C.c_uint32]

P = 0x78000001
BUS_EXEC, BUS_MEMORY, BUS_PC, BUS_VAR_RANGE, BUS_BITWISE = 0, 1, 2, 3, 6
BUS_COMPRESS = 5  # (left[8], right[8], out[8]): out = the first 8 words of Poseidon2(left | right); received by poseidon2_air
OP_ADD, OP_SUB, OP_MUL = 2, 3, 4
LIMB_BITS = (17, 12)  # a pointer or a gap below 2^29 = a 17-bit and a 12-bit limb, both within the variable range checker's 17 bits
PROGRAM_COLUMNS = ["pc", "opcode", "a", "b", "c", "d", "e", "f", "g"]
BOUNDARY_COLUMNS = (["is_valid", "as", "ptr", "p_lo", "p_hi"] + [f"init{i}" for i in range(4)] + ["init_ts"] + [f"fin{i}" for i in range(4)]
                    + ["fin_ts", "same_as", "d_lo", "d_hi"])
BOUNDARY_WIDTH = len(BOUNDARY_COLUMNS)  # 18
CONNECTOR_PUBLIC = ["start_pc", "start_ts", "end_pc", "end_ts"]  # the public values of connector_air(public=True), in this order
CONNECTOR_CONSTRAINTS = [  # pv0 .. pv3 = CONNECTOR_PUBLIC: row 0 is the state the segment starts from, row 1 the one it ends at
    ("start pc", "(1 - is_end) * (pc - pv0)"),
    ("start timestamp", "(1 - is_end) * (timestamp - pv1)"),
    ("end pc", "is_end * (pc - pv2)"),
    ("end timestamp", "is_end * (timestamp - pv3)"),
]
BOUNDARY_CONSTRAINTS = [
    ("is_valid boolean", "is_valid * (is_valid - 1)"),
    ("same_as boolean", "same_as * (same_as - 1)"),
    ("valid rows first", "is_transition * is_valid' * (1 - is_valid)"),
    ("address space 1 or 2", "is_valid * (as - 1) * (as - 2)"),
    ("pointer limbs", "ptr - p_lo - 131072 * p_hi"),
    ("same address space", "is_transition * is_valid' * same_as * (as' - as)"),
    ("next address space", "is_transition * is_valid' * (1 - same_as) * (as' - as - 1)"),
    ("pointer gap", "is_transition * is_valid' * same_as * (ptr' - ptr - 1 - d_lo - 131072 * d_hi)"),
]
NO_CONS = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
STATUS = {0: "written", 1: "cap_log_height too small", 2: "address table bound too small", 3: "a multiplicity that is not +1 or -1",
          4: "a location with only receives or only sends"}


@dataclass
class SystemAir:
    """What `prover.Prover` and `prover.verify_segment` need of one system AIR. fixed: the preprocessed matrix (canonical,
    [pre_width, rows]) or None; log_h: the height the fixed matrix gives the AIR (None: any)."""
    name: str
    width: int
    cons: tuple
    inter: tuple
    columns: list
    pre_width: int = 0
    fixed: np.ndarray | None = None
    transition: bool = False
    log_h: int | None = None
    n_public: int = 0
    _table: torch.Tensor | None = field(default=None, repr=False)

    def fixed_table(self, device="cuda") -> torch.Tensor:
        """the fixed matrix on the device (column-major, Montgomery), uploaded once"""
        if self._table is None:
            self._table = _to_device(self.fixed, device)
        return self._table

    def make_prover(self, num_queries: int = 100, pow_bits: int = 0) -> prover.Prover:
        pre = None
        if self.pre_width:
            pre = (self.fixed_table(), self.pre_width, self.log_h)
            torch.cuda.synchronize()  # the table exists before the prover copies it (on the library's stream)
        return prover.Prover(self.width, self.cons[0], self.cons[1], num_queries=num_queries, pow_bits=pow_bits, interactions=self.inter,
                             preprocessed=pre, transition=self.transition, n_public=self.n_public)

    def description(self, log_h: int | None = None):
        """(width, log_height, cons_bytecode, cons_spans, interactions): an entry of verify_segment's `descs` (transition=True)"""
        return (self.width, self.log_h if log_h is None else log_h, self.cons[0], self.cons[1], self.inter)


def _to_monty(canonical) -> np.ndarray:
    a = np.ascontiguousarray(canonical, dtype=np.uint64).reshape(-1)
    return ((a << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def _to_device(canonical, device="cuda") -> torch.Tensor:
    return torch.from_numpy(_to_monty(canonical).view(np.int32)).to(device)


def _from_device(t: torch.Tensor) -> np.ndarray:
    r_inv = pow(1 << 32, P - 2, P)
    return ((t.cpu().numpy().view(np.uint32).astype(np.uint64) * np.uint64(r_inv)) % np.uint64(P)).astype(np.uint32)


def program_air(table, bus: int = BUS_PC) -> SystemAir:
    """table: the program as canonical words [9, 2^k] (rows pc, opcode, a .. g; a power of two of instructions, padded with rows no
    execution reaches). Main [freq] | preprocessed the nine columns; no constraints; every row is received `freq` times on `bus`."""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    rows = table.shape[1]
    assert table.shape[0] == len(PROGRAM_COLUMNS) and rows >= 2 and rows & (rows - 1) == 0, "the program table is 9 x 2^k words, k >= 1"
    inter = _tables(bus, [(_neg_col(0), [_col(1 + j) for j in range(len(PROGRAM_COLUMNS))])])
    return SystemAir("program", 1, NO_CONS, inter, ["freq"], pre_width=len(PROGRAM_COLUMNS), fixed=table, log_h=rows.bit_length() - 1)


def connector_air(bus: int = BUS_EXEC, public: bool = False) -> SystemAir:
    """Main [pc, timestamp] | preprocessed [is_end] = (0, 1): one interaction with multiplicity 1 - 2 is_end. public: the AIR also has
    the four public values CONNECTOR_PUBLIC and the four degree-2 constraints CONNECTOR_CONSTRAINTS that tie its two rows to them
    (DESIGN.md §5k): the segment proof then SAYS where the execution started and ended (row flags 0: no next row, no selector)."""
    mult = [OP_PUSH_CONST, 1, OP_PUSH_CONST, 2, OP_PUSH_APC, 2, OP_MUL, OP_SUB]
    cons = NO_CONS
    if public:
        rows = prover.row_operands(2, 1)
        # (named operands: the three columns and, as plain operand numbers, the public values)
        col = {"pc": 0, "timestamp": 1, "is_end": 2, **{f"pv{k}": rows.public(k) for k in range(len(CONNECTOR_PUBLIC))}}
        bc, spans = [], []
        for _, text in CONNECTOR_CONSTRAINTS:
            code = air_text.compile_expr(text, col, None)
            spans.append((len(bc), len(code)))
            bc += code
        cons = (np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2))
    return SystemAir("connector", 2, cons, _tables(bus, [(mult, [_col(0), _col(1)])]), ["pc", "timestamp"], pre_width=1,
                     fixed=np.array([[0, 1]], np.uint32), log_h=1, n_public=len(CONNECTOR_PUBLIC) if public else 0)


def connector_links(connector_index: int):
    """The links of prover.verify_segment_chain that make consecutive segments consecutive: the final (pc, timestamp) of one segment's
    public connector (AIR `connector_index` of every segment) is the initial one of the next."""
    i, k = int(connector_index), CONNECTOR_PUBLIC.index
    return [(i, k("end_pc"), i, k("start_pc")), (i, k("end_ts"), i, k("start_ts"))]


def boundary_air(memory_bus: int = BUS_MEMORY, var_range_bus: int = BUS_VAR_RANGE, bitwise_bus: int = BUS_BITWISE, leaf_bus: int | None = None) -> SystemAir:
    """The memory boundary AIR (row-aware: transition=True). Constraints BOUNDARY_CONSTRAINTS; interactions, all on the current row:
    send (as, ptr, init0..3, init_ts), receive (as, ptr, fin0..3, fin_ts), range checks of the four limbs, byte checks of the initial
    words (the final ones are whatever the last access sent, whose chip checked them). leaf_bus (None, the default: the AIR as it
    always was): one more interaction, the send of ((as - 1) * 2^29 + ptr, init0..3, fin0..3) with multiplicity is_valid — the key
    and the four payload words of pw_memory_tree_boundary_leaves, received by the memory Merkle AIR's leaf rows."""
    col = {n: i for i, n in enumerate(BOUNDARY_COLUMNS)}
    rows = prover.row_operands(BOUNDARY_WIDTH)
    bc, spans = [], []
    for _, text in BOUNDARY_CONSTRAINTS:
        code = air_text.compile_expr(text, col, rows)
        spans.append((len(bc), len(code)))
        bc += code
    c = lambda n: _col(col[n])
    const = lambda v: [OP_PUSH_CONST, v]
    valid = c("is_valid")
    by_bus = [
        (memory_bus, [(valid, [c("as"), c("ptr")] + [c(f"init{i}") for i in range(4)] + [c("init_ts")]),
                      (_neg_col(col["is_valid"]), [c("as"), c("ptr")] + [c(f"fin{i}") for i in range(4)] + [c("fin_ts")])]),
        (var_range_bus, [(valid, [c("p_lo"), const(LIMB_BITS[0])]), (valid, [c("p_hi"), const(LIMB_BITS[1])]),
                         (valid, [c("d_lo"), const(LIMB_BITS[0])]), (valid, [c("d_hi"), const(LIMB_BITS[1])])]),
        (bitwise_bus, [(valid, [c("init0"), c("init1"), const(0), const(0)]), (valid, [c("init2"), c("init3"), const(0), const(0)])]),
    ]
    if leaf_bus is not None:
        key = c("as") + const(1) + [OP_SUB] + const(1 << 29) + [OP_MUL] + c("ptr") + [OP_ADD]
        by_bus.append((leaf_bus, [(valid, [key] + [c(f"init{i}") for i in range(4)] + [c(f"fin{i}") for i in range(4)])]))
    return SystemAir("boundary", BOUNDARY_WIDTH, (np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)), _join_tables(by_bus),
                     list(BOUNDARY_COLUMNS), transition=True)


# ---- the Poseidon2 compression chip ---------------------------------------------------------------------------------
# [mult | in[16] | per full round r = 0..7: cube[r][16], sbox[r][16] | per partial round k = 0..12: pcube[k], psbox[k] | out[8]]
P2_FULL_ROUNDS, P2_PARTIAL_ROUNDS, P2_HALF = 8, 13, 4
P2_IN, P2_FULL, P2_PARTIAL, P2_OUT = 1, 17, 17 + 32 * P2_FULL_ROUNDS, 17 + 32 * P2_FULL_ROUNDS + 2 * P2_PARTIAL_ROUNDS
POSEIDON2_WIDTH = P2_OUT + 8  # 307
POSEIDON2_COLUMNS = (["mult"] + [f"in{i}" for i in range(16)]
                     + [f"{n}{r}_{i}" for r in range(P2_FULL_ROUNDS) for n in ("cube", "sbox") for i in range(16)]
                     + [f"{n}{k}" for k in range(P2_PARTIAL_ROUNDS) for n in ("pcube", "psbox")] + [f"out{j}" for j in range(8)])
_M4 = np.array([[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]], np.int64)
# the external layer as one 16 x 16 matrix: M4 on every block of four words, then every word gets its column's sum over the blocks
P2_EXTERNAL = np.kron(np.eye(4, dtype=np.int64), _M4) + np.kron(np.ones((4, 4), np.int64), _M4)


def p2_cube(r: int, i: int) -> int:
    return P2_FULL + 32 * r + i


def p2_sbox(r: int, i: int) -> int:
    return P2_FULL + 32 * r + 16 + i


def _form_code(form, const: int = 0) -> list:
    """one left-leaning sum c0 col0 + c1 col1 + ... + const of a coefficient vector over the columns (never deeper than 3 slots)"""
    code = []
    for c in np.nonzero(form)[0].tolist():
        code += [OP_PUSH_APC, c] + ([OP_PUSH_CONST, int(form[c]), OP_MUL] if int(form[c]) != 1 else []) + ([OP_ADD] if code else [])
    if const or not code:
        code += [OP_PUSH_CONST, int(const)] + ([OP_ADD] if code else [])
    return code


def poseidon2_air(bus: int = BUS_COMPRESS) -> SystemAir:
    """The Poseidon2 compression chip: one permutation per row, 307 main columns POSEIDON2_COLUMNS, no preprocessed columns, no row
    flags, no public values; the tuple (in[0..16], out[0..8]) is received `mult` times on `bus`. The permutation is the library's
    (pw_poseidon2_permute_host): width 16, x^7, an external layer, 4 full, 13 partial, 4 full rounds. Committed per S-box: cube = x^3
    and sbox = cube^2 x, x the linear form that enters it with its round constant — 282 constraints of degree 3 — and out[j] = word j
    of the last external layer (8 of degree 1). The linear layers are applied here, symbolically: a state word is a coefficient
    vector over the committed columns (16 terms in the full rounds, 16 + k in partial round k, 29 entering round 4). A padding row
    is the honest row of the zero input with mult = 0 (no is_valid column).
    THE ROUND CONSTANTS ARE READ FROM prover.poseidon2_constants() NOW and are part of the constraint programs: an AIR made under one
    table is a different AIR under another (its constraints do not hold on rows made under the other) — make it again after
    prover.set_poseidon2_constants."""
    ext_rc, int_rc, diag = (np.asarray(a).astype(np.int64) for a in prover.poseidon2_constants())
    state = np.zeros((16, POSEIDON2_WIDTH), np.int64)  # state[i] = word i as a linear form over the columns
    state[np.arange(16), P2_IN + np.arange(16)] = 1
    bc, spans = [], []

    def constrain(code):
        spans.append((len(bc), len(code)))
        bc.extend(code)

    def sbox(x, cube, out):
        constrain([OP_PUSH_APC, cube] + x + x + [OP_MUL] + x + [OP_MUL, OP_SUB])                       # cube - x^3
        constrain([OP_PUSH_APC, out, OP_PUSH_APC, cube, OP_PUSH_APC, cube, OP_MUL] + x + [OP_MUL, OP_SUB])  # sbox - cube^2 x

    def full_round(r):
        nonlocal state
        for i in range(16):
            sbox(_form_code(state[i], ext_rc[r, i]), p2_cube(r, i), p2_sbox(r, i))
        state = np.zeros((16, POSEIDON2_WIDTH), np.int64)
        state[np.arange(16), [p2_sbox(r, i) for i in range(16)]] = 1
        state = P2_EXTERNAL @ state % P

    state = P2_EXTERNAL @ state % P
    for r in range(P2_HALF):
        full_round(r)
    for k in range(P2_PARTIAL_ROUNDS):
        sbox(_form_code(state[0], int_rc[k]), P2_PARTIAL + 2 * k, P2_PARTIAL + 2 * k + 1)
        state[0] = 0
        state[0, P2_PARTIAL + 2 * k + 1] = 1
        state = (state.sum(axis=0) % P + diag[:, None] * state) % P  # 1 1^T + diag
    for r in range(P2_HALF, P2_FULL_ROUNDS):
        full_round(r)
    for j in range(8):
        constrain([OP_PUSH_APC, P2_OUT + j] + _form_code(state[j]) + [OP_SUB])
    inter = _tables(bus, [(_neg_col(0), [_col(P2_IN + i) for i in range(16)] + [_col(P2_OUT + j) for j in range(8)])])
    return SystemAir("poseidon2", POSEIDON2_WIDTH, (np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)), inter,
                     list(POSEIDON2_COLUMNS))


# ---- traces -------------------------------------------------------------------------------------------------------------------------
def _records(airs):
    return stage.air_records(airs)[0], len(airs)


def _tuple_dict(t) -> dict:
    return dict(bus=int(t.bus), n_args=int(t.n_args), args=[int(x) for x in t.args[:min(t.n_args, prover.PW_BUS_MAX_ARGS)]],
                net_multiplicity=int(t.net_multiplicity), air=int(t.air), interaction=int(t.interaction), row=int(t.row),
                n_contributions=int(t.n_contributions))


def program_frequencies(airs, table: torch.Tensor, log_h: int, pc_base: int, pc_step: int = 4, bus: int = BUS_PC, out: torch.Tensor | None = None):
    """pw_program_frequencies: airs = [(Prover, device trace pointer, log_height)] as for check_segment_buses (the senders); table = the
    program AIR's fixed matrix on the device (SystemAir.fixed_table()). -> (freq: the AIR's main trace, 2^log_h Montgomery words;
    number of foreign tuples; the first of them as a dict, or None). Foreign tuples are in nobody's freq: the caller decides."""
    assert table.numel() == len(PROGRAM_COLUMNS) << log_h
    if out is None:
        out = torch.empty(1 << log_h, dtype=torch.int32, device=table.device)
    assert out.numel() >= 1 << log_h
    recs, n = _records(airs)
    n_foreign, first = C.c_uint64(), prover.PwBusTuple()
    abi.check(lib.pw_program_frequencies(recs, n, bus, pc_base, pc_step, table.data_ptr(), log_h, out.data_ptr(), C.byref(n_foreign), C.byref(first)),
              "pw_program_frequencies")
    return out, int(n_foreign.value), (_tuple_dict(first) if n_foreign.value else None)


def memory_boundary_trace(airs, cap_log_height: int, table_bytes: int = 0, bus: int = BUS_MEMORY, out: torch.Tensor | None = None):
    """pw_memory_boundary_trace -> (trace: 18 x 2^log_height Montgomery words, column-major — None unless status is 0; log_height;
    touched locations; status: a key of STATUS). Status 1: call again with cap_log_height = the log_height returned. The trace pairs
    every location's first receive with its last send and proves nothing: check_segment_buses([... , boundary], buses=[bus]) does."""
    if out is None:
        out = torch.empty(BOUNDARY_WIDTH << cap_log_height, dtype=torch.int32, device="cuda")
    assert out.numel() >= BOUNDARY_WIDTH << cap_log_height
    recs, n = _records(airs)
    lh, locations, status = C.c_uint32(), C.c_uint64(), C.c_uint32()
    abi.check(lib.pw_memory_boundary_trace(recs, n, bus, int(table_bytes), out.data_ptr(), cap_log_height, C.byref(lh), C.byref(locations), C.byref(status)),
              "pw_memory_boundary_trace")
    trace = out[:BOUNDARY_WIDTH << lh.value] if status.value == 0 else None
    return trace, int(lh.value), int(locations.value), int(status.value)


def poseidon2_compress_trace(airs, cap_log_height: int, table_bytes: int = 0, start_log_slots: int = 0, bus: int = BUS_COMPRESS,
                             out: torch.Tensor | None = None):
    """pw_poseidon2_compress_trace: airs = the SENDERS on `bus` as for check_segment_buses -> (trace: 307 x 2^log_height Montgomery
    words, column-major — None unless status is 0; log_height; rows = distinct keys; status: 0 written, 1 cap_log_height too small, 2
    table bound too small). Status 1 is retried once at the height the library asked for, in a buffer of that height — unless the
    caller gave `out`, whose size is the caller's business: then status 1 is returned with the height to come back with.
    The senders' digests are not read: check_segment_buses([..., chip], buses=[bus]) says whether they were right."""
    recs, n = _records(airs)
    own = out is None
    for _ in range(2):
        if own:
            out = torch.empty(POSEIDON2_WIDTH << cap_log_height, dtype=torch.int32, device="cuda")
        assert out.numel() >= POSEIDON2_WIDTH << cap_log_height
        lh, rows, status = C.c_uint32(), C.c_uint64(), C.c_uint32()
        abi.check(lib.pw_poseidon2_compress_trace(recs, n, bus, int(table_bytes), int(start_log_slots), out.data_ptr(), cap_log_height, C.byref(lh),
                                                  C.byref(rows), C.byref(status)), "pw_poseidon2_compress_trace")
        if status.value != 1 or not own:
            break
        cap_log_height = int(lh.value)
    trace = out[:POSEIDON2_WIDTH << lh.value] if status.value == 0 else None
    return trace, int(lh.value), int(rows.value), int(status.value)


def connector_trace(airs, bus: int = BUS_EXEC, with_states: bool = False):
    """The connector's 2 x 2 main trace [pc0, pc1, ts0, ts1] (Montgomery) from what check_segment_buses leaves over on the execution
    bridge: exactly the initial state (received once and never sent) and the final one (sent once and never received).
    with_states: (trace, (pc0, ts0), (pc1, ts1)) — the two tuples as canonical words."""
    _, tuples = prover.check_segment_buses(airs, buses=[bus], tuple_cap=8)
    start = [t for t in tuples if t["net_multiplicity"] == P - 1 and t["n_args"] == 2]
    end = [t for t in tuples if t["net_multiplicity"] == 1 and t["n_args"] == 2]
    if len(tuples) != 2 or len(start) != 1 or len(end) != 1:
        raise ValueError(f"the execution bridge (bus {bus}) does not leave one initial and one final state: {tuples}")
    (pc0, ts0), (pc1, ts1) = start[0]["args"], end[0]["args"]
    trace = _to_device([pc0, pc1, ts0, ts1])
    return (trace, (pc0, ts0), (pc1, ts1)) if with_states else trace


def last_stats() -> dict:
    """pw_system_traces_last_stats of this thread (include/powdr_prover.h PwSystemTraceStats) as a dict, with the scratch bytes held now
    and the most the last call held at once"""
    st = PwSystemTraceStats()
    lib.pw_system_traces_last_stats(C.byref(st))
    out = {n: int(getattr(st, n)) for n, _ in PwSystemTraceStats._fields_}
    out.update(peak_bytes=int(lib.pw_system_traces_peak_bytes()), scratch_bytes=int(lib.pw_system_traces_scratch_bytes()))
    return out


def set_boundary_start_slots(log_slots: int) -> None:
    """pw_memory_boundary_set_start_slots: 2^log_slots slots (6 .. 30) in the first address table of this thread's later
    memory_boundary_trace calls; 0: the default (2^16)"""
    abi.check(lib.pw_memory_boundary_set_start_slots(int(log_slots)), "pw_memory_boundary_set_start_slots")


def close_segment(airs, program_table, pc_base: int, periphery, num_queries: int = 100, pow_bits: int = 0, pc_step: int = 4, table_bytes: int = 0,
                  cap_log_height: int = 16, public_connector: bool = False, poseidon2: bool = False, memory_tree=None):
    """airs: [dict(prover, trace (device tensor), log_h, ...)] — every AIR that sends on the execution bridge, the memory bus and the
    PC lookup, traces made. Appends the program, connector and boundary AIRs as dicts of the same shape (name, role "system", air =
    the SystemAir, width, log_h, cons, inter, trace, prover, pre) and returns the list. periphery (tracegen.Periphery): its histograms
    receive the boundary AIR's range and byte lookups (_apc_apply_bus on its trace) — call this BEFORE the periphery traces are made
    from them. cap_log_height: the boundary buffer first tried (a taller trace is retried once at its own height). public_connector: the connector with its four public values (connector_air(public=True)), set from the two states connector_trace finds; its dict also has public = those values. poseidon2: when any AIR sends on BUS_COMPRESS, the Poseidon2 compression chip (poseidon2_air, made under the constants installed now) is appended after the three, its trace by poseidon2_compress_trace; False (the default): the bus is left alone. Raises on foreign instructions, on a boundary or chip status other than 0 and on an execution bridge that is not a chain.
    memory_tree (a memory_tree.MemoryTree holding the memory the segment starts from; None, the default: the function as it always
    was): the boundary AIR is made with its leaf send (boundary_air(leaf_bus=BUS_LEAF)), its rows' leaves go through the tree's update
    (node ids on) — any status of the update raises, status 3 with the key that does not hold its initial words, and the tree is then
    what it was — and the memory Merkle AIR (memory_tree.merkle_air) is appended after the boundary with its trace
    (memory_tree.merkle_trace) and public = the tree's root before the update | its root after, read from the tree, not from the
    trace. The Merkle AIR is among the senders the Poseidon2 chip's trace is made from, and the chip is appended after it:
    memory_tree needs poseidon2=True (ValueError otherwise, before anything is made — the Merkle AIR's sends on BUS_COMPRESS would
    have no receiver). A segment without a memory location raises before the update (the Merkle AIR has no trace without a root
    row). THE TREE MOVES WITH THE UPDATE: an error raised after it — a Merkle trace or chip status — leaves the tree at the
    segment's final memory, with no segment returned; only the update's own statuses leave it where it was."""
    from .segment_workload import BusReplay

    seg = [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in airs]
    if memory_tree is not None:
        from . import memory_tree as mt  # (it imports this module)

        if not poseidon2:
            raise ValueError("memory_tree needs poseidon2=True: the memory Merkle AIR sends on the compression bus, which the chip receives")
        bnd = boundary_air(leaf_bus=mt.BUS_LEAF)
    else:
        bnd = boundary_air()
    trace, lh, locations, status = memory_boundary_trace(seg, cap_log_height, table_bytes)
    if status == 1:
        trace, lh, locations, status = memory_boundary_trace(seg, lh, table_bytes)
    if status:
        raise ValueError(f"memory boundary: {STATUS[status]} ({locations} locations)")
    BusReplay(bnd.inter, 1 << lh)(trace.data_ptr(), periphery)
    prog = program_air(program_table)
    freq, n_foreign, first = program_frequencies(seg, prog.fixed_table(), prog.log_h, pc_base, pc_step)
    if n_foreign:
        raise ValueError(f"{n_foreign} executed instructions are not in the program, the first: {first}")
    con = connector_air(public=public_connector)
    con_trace, start, end = connector_trace(seg, with_states=True)
    system = [(prog, freq, prog.log_h), (con, con_trace, 1), (bnd, trace, lh)]
    public, made = {con.name: np.array([*start, *end], np.uint32)}, {}
    hashers = any(BUS_COMPRESS in np.asarray(a["inter"][0]).reshape(-1, 3)[:, 0] for a in airs if a.get("inter") is not None)
    if memory_tree is not None:
        if not locations:
            raise ValueError(f"memory Merkle trace: {mt.MERKLE_STATUS[2]}")
        mk = mt.merkle_air(memory_tree.height)
        root_before = memory_tree.root()
        keys, init, fin = mt.boundary_leaves(trace, lh, locations)
        t_status, info, records, rec_lh, rec_rows = memory_tree.update(keys, init, fin, node_ids=True)
        if t_status:
            raise ValueError(f"memory tree: status {t_status}, {mt.STATUS[t_status]}" + (f" (key {info})" if t_status == 3 else f" ({info})"))
        mk_trace, mk_lh, nodes, mk_status = mt.merkle_trace(*records, rec_lh, rec_rows, memory_tree.height)
        if mk_status:
            raise ValueError(f"memory Merkle trace: {mt.MERKLE_STATUS[mk_status]} ({nodes} nodes)")
        public[mk.name] = np.concatenate([root_before, memory_tree.root()]).astype(np.uint32)
        made[mk.name] = mk.make_prover(num_queries, pow_bits)
        system.append((mk, mk_trace, mk_lh))
        seg = seg + [(made[mk.name], mk_trace.data_ptr(), mk_lh)]  # the chip's senders
        hashers = True
    if poseidon2 and hashers:
        p2_trace, p2_lh, p2_rows, p2_status = poseidon2_compress_trace(seg, min(cap_log_height, 10), table_bytes)
        if p2_status:
            raise ValueError(f"poseidon2 chip: {STATUS[p2_status]} ({p2_rows} rows)")
        system.append((poseidon2_air(), p2_trace, p2_lh))
    out = list(airs)
    for air, t, h in system:
        p = made.get(air.name) or air.make_prover(num_queries, pow_bits)
        out.append(dict(name=air.name, role="system", air=air, width=air.width, log_h=h, cons=air.cons, inter=air.inter, trace=t, prover=p,
                        pre=(air.fixed_table(), air.pre_width, air.log_h) if air.pre_width else None))
        if air.n_public:
            out[-1]["public"] = public[air.name]
            p.set_public_values(out[-1]["public"])
    return out
