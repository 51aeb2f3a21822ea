"""The second route of the APC call selection, written from the semantics of the reference's
autoprecompiles/src/execution/{evaluator,candidates}.rs: an evaluator that steps through an APC's optimistic constraints state by state
with a memory of fetched values, a candidate tracker with `try_insert` / `check_conditions` / `abort_in_progress` / `extract_calls`
that folds the done candidates of a batch pair by pair, and the driver the reference's unit tests use on top. No component shortcut:
batches are exactly those the tracker meets. Plain Python, no GPU.

A state is (pc, regs, clk). Operands: ("num", v) | ("pc", instr_idx) | ("reg", instr_idx, reg, limb)."""
from __future__ import annotations

COUNTERS = ("matches", "refused", "failed", "aborted", "done", "discarded", "calls")


def literals(c):
    out = []
    for e in c:
        if e[0] != "num" and e not in out:
            out.append(e)
    return out


def fetch_of(lit):
    return ("pc",) if lit[0] == "pc" else ("reg", lit[2])


class Constraints:
    """grouped by step: `checks[step]` the constraints first evaluable there, `fetches[step]` what later constraints read of it"""

    def __init__(self, constraints=()):
        self.fetches, self.checks = {}, {}
        for c in constraints:
            c = (tuple(c[0]), tuple(c[1]))
            lits = literals(c)
            step = max((l[1] for l in lits), default=0)
            for l in lits:
                if step > l[1]:
                    self.fetches.setdefault(l[1], []).append(fetch_of(l))
            self.checks.setdefault(step, []).append(c)


def fetch(f, state):
    return state[0] if f[0] == "pc" else state[1][f[1]]


class Evaluator:
    def __init__(self, limb_bits=8):
        self.instruction_index, self.memory, self.limb_bits = 0, {}, limb_bits

    def value(self, e, state):
        if e[0] == "num":
            return e[1]
        f = fetch_of(e)
        v = fetch(f, state) if e[1] == self.instruction_index else self.memory[(e[1], f)]
        if e[0] == "reg":
            v = (v >> (e[3] * self.limb_bits)) & ((1 << self.limb_bits) - 1)
        return v

    def try_next_execution_step(self, state, cons: Constraints) -> bool:
        for left, right in cons.checks.get(self.instruction_index, ()):
            if self.value(left, state) != self.value(right, state):
                return False
        for f in cons.fetches.get(self.instruction_index, ()):
            self.memory[(self.instruction_index, f)] = fetch(f, state)
        self.instruction_index += 1
        return True


class Candidate:
    __slots__ = ("apc_id", "start", "end", "evaluator", "total", "dead")

    def __init__(self, apc_id, start, evaluator, total):
        self.apc_id, self.start, self.end, self.evaluator, self.total, self.dead = apc_id, start, None, evaluator, total, False


class ApcCandidates:
    """apcs: [{"cycle_count", "priority", "constraints": Constraints}]. `candidates` holds the live ones in insertion order, `in_progress`
    those whose evaluator still runs (the same objects); a failed candidate leaves both."""

    def __init__(self, apcs, limb_bits=8):
        self.apcs, self.limb_bits = apcs, limb_bits
        self.candidates, self.in_progress = [], []
        self.last_discarded = []

    def try_insert(self, state, apc_id) -> bool:
        ev = Evaluator(self.limb_bits)
        if not ev.try_next_execution_step(state, self.apcs[apc_id]["constraints"]):
            return False
        c = Candidate(apc_id, state[2], ev, self.apcs[apc_id]["cycle_count"] + 1)
        self.candidates.append(c)
        self.in_progress.append(c)
        return True

    def check_conditions(self, state) -> list:
        """-> the apc ids of the candidates that failed at this state"""
        failed, still = [], []
        for c in self.in_progress:
            if not c.evaluator.try_next_execution_step(state, self.apcs[c.apc_id]["constraints"]):
                c.dead = True
                failed.append(c.apc_id)
            elif c.total == c.evaluator.instruction_index:
                c.end, c.evaluator = state[2], None
            else:
                still.append(c)
        if failed:
            self.candidates = [c for c in self.candidates if not c.dead]
        self.in_progress = still
        return failed

    def abort_in_progress(self) -> list:
        out = [c.apc_id for c in self.in_progress]
        for c in self.in_progress:
            c.dead = True
        self.candidates = [c for c in self.candidates if not c.dead]
        self.in_progress = []
        return out

    def count_done(self):
        return sum(1 for c in self.candidates if c.end is not None)

    def count_in_progress(self):
        return len(self.in_progress)

    def extract_calls(self) -> list:
        """[(apc_id, from, to)] once nothing is in progress: all pairs (i < j) in order, the lower rank of an overlapping live pair is
        discarded; rank = (priority, length, earlier insertion). Insertion order is start order, so the inner loop stops at the first j
        that starts at or after i's end: no later one overlaps i."""
        self.last_discarded = []
        if self.in_progress:
            return []
        cs = self.candidates
        rank = [(self.apcs[c.apc_id]["priority"], c.end - c.start, -k) for k, c in enumerate(cs)]
        discard = [False] * len(cs)
        for i in range(len(cs)):
            for j in range(i + 1, len(cs)):
                if cs[j].start >= cs[i].end:
                    break
                if discard[i] or discard[j] or not (cs[i].start < cs[j].end and cs[j].start < cs[i].end):
                    continue
                if rank[i] > rank[j]:
                    discard[j] = True
                else:
                    discard[i] = True
        self.candidates = []
        self.last_discarded = [c.apc_id for c, d in zip(cs, discard) if d]
        return [(c.apc_id, c.start, c.end) for c, d in zip(cs, discard) if not d]


def make_apcs(apcs):
    """[(start_pc, cycle_count, priority, constraints)] -> the tracker's table"""
    return [{"start_pc": a[0], "cycle_count": a[1], "priority": a[2], "constraints": Constraints(a[3] if len(a) > 3 else ())} for a in apcs]


def select(pcs, apcs, regs=None, limb_bits=8):
    """The driver: for every state check_conditions, extract_calls, then try_insert of every APC that starts at the state's pc in
    ascending apc_id; after the last state abort_in_progress and extract_calls. pcs: the N + 1 pcs; regs: one row per register.
    -> {"calls": [(apc_id, from, to)], "counters": [per APC {...}], "covered": positions inside calls}"""
    table = make_apcs(apcs)
    by_pc = {}
    for a, apc in enumerate(table):
        by_pc.setdefault(apc["start_pc"], []).append(a)
    tracker = ApcCandidates(table, limb_bits)
    counters = [dict.fromkeys(COUNTERS, 0) for _ in table]
    calls = []

    def extract():
        done = [c.apc_id for c in tracker.candidates] if not tracker.in_progress else []
        got = tracker.extract_calls()
        if done or got:
            for a in done:
                counters[a]["done"] += 1
            for a in tracker.last_discarded:
                counters[a]["discarded"] += 1
            for a, _, _ in got:
                counters[a]["calls"] += 1
            calls.extend(got)

    n_regs = len(regs) if regs is not None else 0
    for i, pc in enumerate(pcs):
        state = (pc, tuple(regs[r][i] for r in range(n_regs)), i)
        for a in tracker.check_conditions(state):
            counters[a]["failed"] += 1
        extract()
        for a in by_pc.get(pc, ()):
            counters[a]["matches"] += 1
            if not tracker.try_insert(state, a):
                counters[a]["refused"] += 1
    for a in tracker.abort_in_progress():
        counters[a]["aborted"] += 1
    extract()
    return {"calls": calls, "counters": counters, "covered": sum(e - s for _, s, e in calls)}


# ---- shared by the tests ----------------------------------------------------------------------------------------------------------------
def operand_from_serde(j):
    if "Number" in j:
        return ("num", j["Number"])
    lit = j["Literal"]
    return ("pc", lit["instr_idx"]) if lit["val"] == "Pc" else ("reg", lit["instr_idx"], lit["val"]["RegisterLimb"][0], lit["val"]["RegisterLimb"][1])


def constraints_from_serde(cs):
    return [(operand_from_serde(c["left"]), operand_from_serde(c["right"])) for c in cs]


# the two order traps as (pcs, apcs, calls): start pcs 10, 20, 30 mark where A, B, C start in an execution of otherwise distinct pcs
def trap(ranges_priorities, n=8):
    pcs = [100 + i for i in range(n)]
    apcs = []
    for k, (start, end, priority) in enumerate(ranges_priorities):
        pcs[start] = 10 * (k + 1)
        apcs.append((10 * (k + 1), end - start, priority, []))
    return pcs, apcs


TRAPS = {
    # A is discarded by B, B by C: the fold is not "best rank first", which would keep A next to C
    "chain": (trap([(0, 3, 1), (2, 5, 2), (4, 7, 3)]), [(2, 4, 7)]),
    # A discards B, then meets C and is discarded: B stays discarded although nothing that survives overlaps it
    "eaten follower": (trap([(0, 4, 2), (1, 3, 1), (3, 6, 3)]), [(2, 3, 6)]),
}
