"""TEST INFRASTRUCTURE — a CHAINED executor for the system AIRs: one block that ends with a jump back to its first
instruction is executed N times with PERSISTENT registers and memory, call k + 1 starting at the timestamp call k ended at, so that
the records of all calls form one consistent execution — every access finds the word and the timestamp the previous access to that
location left, the execution bridge is one chain, every executed instruction is a row of one program. (oracle.rv32_vm.execute_block
draws every call's state afresh: its calls do not chain.) Results come from oracle.original_chips.rv32_model, the access order from
oracle.rv32_vm.access_list. Only a location touched for the first time draws its initial (word, timestamp).

The block has no branch and keeps its pointer aligned and small, so no call can leave its path: nothing is ever redrawn."""
import numpy as np

from oracle import original_chips as oc
from oracle import rv32_vm

M32 = 0xFFFFFFFF
START_PC = 0x200000
X = lambda n: 4 * n  # register pointer

# [opcode, a, b, c, d, e, f, g]: six chips (BaseAlu, LoadStore, LessThan, Shift, Multiplication, JalLui). x2 counts the calls (written
# in one call, read in the next); x1 walks through memory one word per call: a call loads the word the previous call stored at 4(x1)
# and stores to fresh memory, so memory locations are touched once (the last store), twice, and registers by every call.
BLOCK = [
    [512, X(2), X(2), 1, 1, 0, 0, 0],        # ADDI  x2 = x2 + 1
    [528, X(3), X(1), 0, 1, 2, 1, 0],        # LOADW x3 = [x1 + 0]            (address space 2)
    [512, X(3), X(3), X(2), 1, 1, 0, 0],     # ADD   x3 = x3 + x2
    [531, X(3), X(1), 4, 1, 2, 1, 0],        # STOREW [x1 + 4] = x3
    [521, X(4), X(3), X(2), 1, 1, 0, 0],     # SLTU  x4 = x3 < x2
    [517, X(6), X(3), 3, 1, 0, 0, 0],        # SLLI  x6 = x3 << 3
    [592, X(7), X(3), X(2), 1, 0, 0, 0],     # MUL   x7 = x3 * x2
    [514, X(5), X(6), X(7), 1, 1, 0, 0],     # XOR   x5 = x6 ^ x7
    [512, X(1), X(1), 4, 1, 0, 0, 0],        # ADDI  x1 = x1 + 4
    [560, 0, 0, oc.P - 36, 1, 0, 0, 0],      # JAL   x0, -36: back to the first instruction, nothing written
]


class Execution:
    """table, rbs (rows per call and kind), wpc: oc.build_instruction_table of the block; rec u32[wpc, calls]: the call records;
    initial / final {(as, ptr): (word, timestamp)}: every touched location before its first and after its last access; start / end:
    the (pc, timestamp) the execution begins and ends at; accesses: the number of enabled accesses."""

    def __init__(self, calls, seed=0, block=BLOCK, start_pc=START_PC):
        self.block, self.start_pc, self.calls = block, start_pc, calls
        self.table, _, self.rbs, self.wpc = oc.build_instruction_table(block, [True] * len(block), start_pc)
        rng = np.random.default_rng([seed, 0x5e9])
        ts = int(rng.integers(1 << 10, 1 << 12))
        self.start = (start_pc, ts)
        state, self.initial = {}, {}
        first_ts = ts

        def touch(space, ptr, want=None):
            key = (space, ptr)
            if key not in state:
                word = int(rng.integers(0, 1 << 32)) if want is None else want
                if key == (1, 0):
                    word = 0  # x0 holds 0
                state[key] = self.initial[key] = (word & M32, int(rng.integers(0, first_ts)))
            return state[key]

        next_pcs = [start_pc + 4 * (i + 1) for i in range(len(block) - 1)] + [start_pc]
        self.rec = np.zeros((self.wpc, calls), np.uint32)
        self.accesses = 0
        for call in range(calls):
            col = self.rec[:, call:call + 1]
            col[0, 0] = ts
            for i, ins in enumerate(self.table):
                k, op, o = int(ins["kind"]), int(ins["opcode"]), int(ins["rec_off"])
                t = ts + int(ins["ts_delta"])
                n_data = oc.RECORD_WORDS[k] - oc.N_PREV_TS[k]
                mem_ptr = None
                if k in (oc.KIND_LOAD_STORE, oc.KIND_LOAD_SIGN_EXTEND):
                    key = (1, int(ins["b"]))
                    if key not in state:  # the base register's first read: a legal, aligned pointer with room for every call
                        touch(*key, int(rng.integers(1 << 10, 1 << 20)) * 4)
                    ptr = (touch(*key)[0] + oc._imm_ext(ins)) & M32
                    assert ptr < 1 << 29 and not ptr & oc.ACCESS_ALIGN[op], "the block left the ISA's domain (no redraws here)"
                    mem_ptr = ptr & ~3
                accesses = rv32_vm.access_list(ins, mem_ptr)
                for j, (enabled, space, ptr) in enumerate(accesses):
                    if enabled:
                        word, last = touch(space, ptr)
                        col[o + j, 0] = word
                        col[o + n_data + j, 0] = last
                        for jj in range(j):  # an earlier access of THIS instruction to the same location moved its timestamp
                            if accesses[jj][0] and accesses[jj][1:] == (space, ptr):
                                col[o + n_data + j, 0] = t + jj
                model, next_pc, step = oc.rv32_model(ins, col, col[0])
                assert step == len(accesses) == len(model)
                for j, ((enabled, space, ptr), (m_en, m_space, m_ptr, before, after)) in enumerate(zip(accesses, model)):
                    assert enabled == m_en and (not enabled or (space == m_space and ptr == int(m_ptr[0])))
                    if enabled:
                        state[(space, ptr)] = (int(after[0]) & M32, t + j)
                        self.accesses += 1
                assert int(next_pc[0]) == next_pcs[i] % oc.P, "the block left its path (no redraws here)"
            ts += sum(oc.TS_STEP[int(ins["kind"])] for ins in self.table)
        self.final = dict(state)
        self.end = (start_pc, ts)

    def program_table(self):
        """canonical [9, 2^k]: the block's instructions as rows (pc, opcode, a, b, c, d, e, f, g), padded to a power of two (at least 16
        rows) with rows of opcode 0 at the following pcs, which nothing executes"""
        n = len(self.block)
        rows = max(16, 1 << (n - 1).bit_length())
        t = np.zeros((9, rows), np.uint32)
        t[0] = self.start_pc + 4 * np.arange(rows)
        for i, ins in enumerate(self.block):
            t[1:, i] = [int(x) % oc.P for x in ins]
        return t

    def instruction_airs(self):
        """[(kind name, canonical trace [width, height], (constraint bytecode, spans, interactions))] of the instruction AIRs the block uses, rows by the numpy
        restatement (oracle.original_chips.expand_dummy_traces)"""
        from powdr_amd import synth

        traces = oc.expand_dummy_traces(self.table, self.rec, self.rbs)
        return [(oc.KIND_NAMES[k], t, synth.reference_air_programs(oc.KIND_NAMES[k])) for k, t in sorted(traces.items())]
