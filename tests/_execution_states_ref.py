"""TEST INFRASTRUCTURE — the second route to the states of an execution, written from the definition with numpy,
dictionaries and bisect: the bridge gives positions, time keys and pcs (tests/_empirical_ref.py `bridge`, the trace route's own
restatement), the memory bus's interactions — evaluated with oracle.original_chips.eval_postfix, as tests/_bus_multiset.py `tally`
evaluates them — give the registers. And a synthetic "state log" AIR with a generator of consistent random executions.

The definition. State i < N is the machine before the active row with the i-th smallest timestamp ts_i, state N the machine after the
last one. A register access is an active interaction on the memory bus (as, ptr, d0..d3, t) with as == reg_as; the address space is
looked at first, then the multiplicity (+-1 or status 8), then ptr (a multiple of the step or status 8), then whether anybody asked for
register ptr / step (if not: skipped), then the data words (below 256 or status 8). A send (+1) with timestamp t is seen from state
p = #{j : ts_j <= t} on (p = 0: status 8); two sends with one (register, t): status 8; of the sends to one register with one p the
largest t wins. Per register the receive (-1) with the smallest previous timestamp (then the smallest word) holds the value at state 0."""
import bisect

import numpy as np

from oracle import original_chips as ooc
from tests import _empirical_ref as eref

P = ooc.P
Status = eref.Status
ROW_BITS, INTERACTION_BITS = 26, 20
OP_COL, OP_CONST, OP_ADD, OP_NEG = 0, 1, 2, 5


def pack_witness(air, interaction, row):
    return (air << (ROW_BITS + INTERACTION_BITS)) | (interaction << ROW_BITS) | row


def positions(airs, final_pc, segments=None, bus=0):
    """-> (timestamps ascending, pcs of the N + 1 states, time keys); raises Status 7, then 4"""
    rows, worst = [], None
    for a, (cols, interactions) in enumerate(airs):
        got = eref.bridge(cols, interactions, bus) if interactions is not None else None
        if got is None:
            continue
        active, bad, pc, ts = got
        if bad.any():
            w = (a << 32) | int(np.nonzero(bad)[0][0])
            worst = w if worst is None else min(worst, w)
        rows += [(int(ts[r]), int(pc[r])) for r in np.nonzero(active & ~bad)[0].tolist()]
    if worst is not None:
        raise Status(7, worst)
    seg = 0 if segments is None or not len(segments) else int(segments[0])
    rows.sort()
    ts = [t for t, _ in rows]
    dup = [t for t, n in zip(ts, ts[1:]) if t == n]
    if dup:
        raise Status(4, (seg << 32) | min(dup))
    return ts, [pc for _, pc in rows] + [int(final_pc)], [(seg << 32) | t for t in ts]


def register_accesses(airs, wanted, memory_bus=1, reg_as=1, ptr_step=4):
    """-> (sends [(register, t, word, witness)], receives [(register, previous ts, word)], bad witnesses, accessed registers wanted or not)"""
    sends, receives, bad, seen = [], [], [], set()
    for a, (cols, interactions) in enumerate(airs):
        if interactions is None:
            continue
        cols = [np.asarray(c).astype(np.int64) for c in cols]
        rows = len(cols[0])
        inter = np.asarray(interactions[0], dtype=np.int64).reshape(-1, 3)
        spans = np.asarray(interactions[1], dtype=np.int64).reshape(-1, 2)
        bc = np.asarray(interactions[2])

        def value(span):
            off, ln = spans[span]
            return np.broadcast_to(np.asarray(ooc.eval_postfix(bc[off:off + ln], cols), dtype=np.int64) % P, (rows,))

        for i, (bus, n_args, first) in enumerate(inter.tolist()):
            if bus % P != memory_bus:
                continue
            assert n_args == 7
            m = value(first)
            on = np.nonzero((m != 0) & (value(first + 1) == reg_as))[0]
            if not len(on):
                continue
            args = np.stack([value(first + 2 + j)[on] for j in range(6)], axis=1).tolist()
            for r, mult, (ptr, d0, d1, d2, d3, t) in zip(on.tolist(), m[on].tolist(), args):
                if mult not in (1, P - 1) or ptr % ptr_step:
                    bad.append((a, i, r))
                    continue
                reg = ptr // ptr_step
                seen.add(reg)
                if reg not in wanted:
                    continue
                if max(d0, d1, d2, d3) >= 256:
                    bad.append((a, i, r))
                    continue
                word = d0 | d1 << 8 | d2 << 16 | d3 << 24
                if mult == 1:
                    sends.append((reg, t, word, (a, i, r)))
                else:
                    receives.append((reg, t, word))
    return sends, receives, bad, seen


def states(airs, regs, final_pc, initial_regs=None, segments=None, bus=0, memory_bus=1, reg_as=1, ptr_step=4):
    """-> dict(pcs [N + 1], regs u32[len(regs), N + 1], time_keys [N], sends, accessed); raises Status(7 | 4 | 8 | 9 | 10, info)"""
    regs = [int(r) for r in regs]
    ts, pcs, keys = positions(airs, final_pc, segments, bus)
    n_states = len(pcs)
    sends, receives, bad, seen = register_accesses(airs, set(regs), memory_bus, reg_as, ptr_step)
    once = {}
    for reg, t, word, w in sends:
        once.setdefault((reg, t), []).append(w)
    writes = {}  # (register, p) -> (t, word)
    for reg, t, word, w in sends:
        p = bisect.bisect_right(ts, t)
        if p == 0 or len(once[(reg, t)]) > 1:
            bad.append(w)
            continue
        writes[(reg, p)] = max(writes.get((reg, p), (-1, 0)), (t, word))
    if bad:
        raise Status(8, pack_witness(*min(bad)))
    first = {}
    for reg, t, word in receives:
        first[reg] = min(first.get(reg, (P, 0)), (t, word))
    if initial_regs is None:
        none = [r for r in regs if r not in first]
        if none:
            raise Status(9, min(none))
        at0 = [first[r][1] for r in regs]
    else:
        at0 = [int(w) for w in initial_regs]
        wrong = [r for r, w in zip(regs, at0) if r in first and first[r][1] != w]
        if wrong:
            raise Status(10, min(wrong))
    table = np.zeros((len(regs), n_states), np.uint32)
    for k, reg in enumerate(regs):
        value = np.full(n_states, -1, np.int64)
        value[0] = at0[k]
        for (r, p), (_, word) in writes.items():
            if r == reg:
                value[p] = word
        last = np.maximum.accumulate(np.where(value >= 0, np.arange(n_states), 0))
        table[k] = value[last]
    return dict(pcs=pcs, regs=table, time_keys=keys, sends=len(sends), accessed=seen)


# ---- the state log AIR ------------------------------------------------------------------------------------------------------------------
# columns: is_valid, pc, ts, next_pc, next_ts, then per access: en, as, ptr, prev0..3, prev_ts, new0..3
HEAD, PER_ACCESS = 5, 12


def state_log_interactions(n_access, bus=0, memory_bus=1):
    """bridge: receive -is_valid of (pc, ts), send +is_valid of (next_pc, next_ts); per access j a memory receive -en of
    (as, ptr, prev0..3, prev_ts) and a send +en of (as, ptr, new0..3, ts + j)"""
    col = lambda c: [OP_COL, c]
    inter, spans, bc = [], [], []

    def add(b, programs):
        inter.append((b, len(programs) - 1, len(spans)))
        for prog in programs:
            spans.append((len(bc), len(prog)))
            bc.extend(prog)

    add(bus, [col(0) + [OP_NEG], col(1), col(2)])
    add(bus, [col(0), col(3), col(4)])
    for j in range(n_access):
        c = HEAD + PER_ACCESS * j
        add(memory_bus, [col(c) + [OP_NEG], col(c + 1), col(c + 2)] + [col(c + 3 + k) for k in range(4)] + [col(c + 7)])
        add(memory_bus, [col(c), col(c + 1), col(c + 2)] + [col(c + 8 + k) for k in range(4)] + [col(2) + [OP_CONST, j, OP_ADD]])
    return np.array(inter, np.uint32).reshape(-1, 3), np.array(spans, np.uint32).reshape(-1, 2), np.array(bc, np.uint32)


def state_log(rows, n_access, log_h=None, places=None):
    """rows: [(pc, ts, next_pc, next_ts, [(en, as, ptr, prev word, prev ts, new word)])] -> cols [5 + 12 * n_access, 2^log_h] canonical:
    row k at position places[k] (default k), zeros elsewhere"""
    n = len(rows)
    log_h = max(1, (max(n, 2) - 1).bit_length()) if log_h is None else log_h
    cols = np.zeros((HEAD + PER_ACCESS * n_access, 1 << log_h), np.uint32)
    at = np.arange(n) if places is None else np.asarray(places)
    assert len(at) == n and len(set(at.tolist())) == n and (n == 0 or at.max() < 1 << log_h)
    for k, (pc, ts, next_pc, next_ts, accesses) in zip(at.tolist(), rows):
        cols[:HEAD, k] = [1, pc, ts, next_pc, next_ts]
        assert len(accesses) <= n_access
        for j, (en, space, ptr, prev, prev_ts, new) in enumerate(accesses):
            c = HEAD + PER_ACCESS * j
            cols[c:c + PER_ACCESS, k] = [en, space, ptr] + [(prev >> 8 * b) & 255 for b in range(4)] + [prev_ts] + [(new >> 8 * b) & 255 for b in range(4)]
    return cols


class Execution:
    """A consistent execution of n instructions over registers 0 .. n_regs - 1 (address space 1, pointer 4 * register) and as many
    words of address space 2 at the SAME pointers. plan(i) -> the accesses of instruction i as [(space, register, new word or None =
    read)]; default: up to n_access random accesses, half of them reads, a quarter of them to address space 2. Instruction i has
    timestamp ts0 + gap * i and its access j the timestamp + j.
    rows: state_log's rows in time order; truth u32[n_regs, n + 1]: every register at every state; initial: the registers at state 0;
    pcs: the n + 1 pcs; accessed: the registers touched."""

    def __init__(self, n, seed=0, n_regs=6, n_access=3, plan=None, ts0=1000, gap=None):
        rng = np.random.default_rng([seed, 0x57a7e])
        gap = n_access if gap is None else gap
        assert gap >= n_access
        self.n, self.n_regs, self.n_access = n, n_regs, n_access
        word = lambda: int(rng.integers(0, 1 << 32))
        mem = {(s, 4 * r): (word(), int(rng.integers(0, ts0))) for s in (1, 2) for r in range(n_regs)}
        self.initial = [mem[(1, 4 * r)][0] for r in range(n_regs)]
        pcs = (4 * rng.integers(0, 5, size=n + 1)).tolist()
        self.pcs, self.rows, self.accessed = pcs, [], set()
        truth = np.zeros((n_regs, n + 1), np.uint32)
        for i in range(n):
            truth[:, i] = [mem[(1, 4 * r)][0] for r in range(n_regs)]
            ts = ts0 + gap * i
            if plan is None:
                todo = [(2 if rng.integers(0, 4) == 0 else 1, int(rng.integers(0, n_regs)), None if rng.integers(0, 2) else word())
                        for _ in range(int(rng.integers(0, n_access + 1)))]
            else:
                todo = plan(i)
            accesses = []
            for j, (space, reg, new) in enumerate(todo):
                prev, prev_ts = mem[(space, 4 * reg)]
                new = prev if new is None else int(new) & 0xFFFFFFFF
                accesses.append((1, space, 4 * reg, prev, prev_ts, new))
                mem[(space, 4 * reg)] = (new, ts + j)
                if space == 1:
                    self.accessed.add(reg)
            self.rows.append((pcs[i], ts, pcs[i + 1], ts + gap, accesses))
        truth[:, n] = [mem[(1, 4 * r)][0] for r in range(n_regs)]
        self.truth, self.final_pc = truth, pcs[n]

    def airs(self, seed=1, split=True):
        """the rows at random places of two state-log AIRs of different heights (or in order in one)"""
        it = state_log_interactions(self.n_access)
        if not split:
            return [(state_log(self.rows, self.n_access), it)]
        rng = np.random.default_rng([seed, self.n])
        side = rng.integers(0, 3, size=self.n) == 0  # about a third of the rows in the smaller AIR
        parts = [[r for r, s in zip(self.rows, side) if not s], [r for r, s in zip(self.rows, side) if s]]
        out = []
        for part, extra in zip(parts, (1, 0)):
            log_h = max(1, (max(len(part), 2) - 1).bit_length()) + extra
            out.append((state_log(part, self.n_access, log_h=log_h, places=rng.permutation(1 << log_h)[:len(part)]), it))
        return out
