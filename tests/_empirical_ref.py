"""TEST INFRASTRUCTURE — the second route to the empirical constraints, written from the definition with dictionaries
and Python sorting: no fingerprints, no sort by key pairs, a sequential walk over the rows in time order. And a tiny "block log" AIR
for synthetic rows: main columns [is_valid, pc, ts, data...], a bus-0 receive -is_valid of (pc, ts) and a send +is_valid of (pc, ts)."""
import numpy as np

from oracle import original_chips as ooc

P = ooc.P
OP_PUSH_APC, OP_NEG = 0, 5


class Status(Exception):
    def __init__(self, status, info):
        super().__init__(f"status {status}, info {info}")
        self.status, self.info = status, info


def percentile_indices(n):
    return n // 100, n * 99 // 100


def detect_rows(rows, blocks, pc_step=4):
    """rows: [(air, segment, timestamp, pc, [cells])] in any order -> dict(column_ranges_by_pc, equivalence_classes_by_block, pc_counts,
    air_id_by_pc); raises Status(4 | 3 | 5, info)"""
    rows = sorted(rows, key=lambda r: (r[1] << 32) | r[2])
    keys = [(r[1] << 32) | r[2] for r in rows]
    dup = [k for k, n in zip(keys, keys[1:]) if k == n]
    if dup:
        raise Status(4, min(dup))
    start_of = {int(s): int(n) for s, n in blocks}
    inside = {int(s) + k * pc_step for s, n in blocks for k in range(1, int(n))}
    instances = {}  # start pc -> [instance = list of rows]
    i = 0
    while i < len(rows):
        pc = rows[i][3]
        if pc in start_of:
            n = start_of[pc]
            inst = rows[i:i + n]
            if len(inst) < n or any(r[3] != pc + k * pc_step for k, r in enumerate(inst)):
                raise Status(3, keys[i])
            instances.setdefault(pc, []).append(inst)
            i += n
        elif pc in inside:
            raise Status(3, keys[i])  # an instruction of a listed block without its head
        else:
            i += 1
    by_pc = {}
    for r in rows:
        by_pc.setdefault(r[3], []).append(r)
    two = [pc for pc, rs in by_pc.items() if len({r[0] for r in rs}) > 1]
    if two:
        raise Status(5, min(two))
    ranges, counts, air_of = {}, {}, {}
    for pc, rs in sorted(by_pc.items()):
        n = len(rs)
        lo, hi = percentile_indices(n)
        cols = [sorted(int(r[4][c]) for r in rs) for c in range(len(rs[0][4]))]
        ranges[pc] = [(v[lo], v[hi]) for v in cols]
        counts[pc] = n
        air_of[pc] = rs[0][0]
    classes = {}
    for start, insts in sorted(instances.items()):
        groups = {}
        for k in range(start_of[start]):
            for c in range(len(insts[0][k][4])):
                groups.setdefault(tuple(int(inst[k][4][c]) for inst in insts), []).append((k, c))
        classes[start] = sorted(sorted(g) for g in groups.values() if len(g) >= 2)
    return dict(column_ranges_by_pc=ranges, equivalence_classes_by_block=classes, pc_counts=counts, air_id_by_pc=air_of)


def bridge(cols, interactions, bus=0):
    """the interactions on `bus` of one host AIR, row by row -> (active mask, bad mask, pc, ts)"""
    cols = [np.asarray(c).astype(np.int64) for c in cols]
    rows = len(cols[0])
    inter = np.asarray(interactions[0], dtype=np.int64).reshape(-1, 3)
    spans = np.asarray(interactions[1], dtype=np.int64).reshape(-1, 2)
    bc = np.asarray(interactions[2])

    def value(span):
        off, ln = spans[span]
        return np.broadcast_to(np.asarray(ooc.eval_postfix(bc[off:off + ln], cols), dtype=np.int64) % P, (rows,)).copy()

    active, bad, n_recv = np.zeros(rows, bool), np.zeros(rows, bool), np.zeros(rows, np.int64)
    pc, ts = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    found = False
    for b, n_args, first in inter.tolist():
        if b % P != bus:
            continue
        found = True
        assert n_args == 2
        m = value(first)
        active |= m != 0
        recv = m == P - 1
        bad |= (m != 0) & ~recv & (m != 1)
        take = recv & (n_recv == 0)
        pc[take], ts[take] = value(first + 1)[take], value(first + 2)[take]
        n_recv += recv
    bad |= active & (n_recv != 1)
    return (active, bad, pc, ts) if found else None


def detect(airs, blocks, segments=None, bus=0, pc_step=4, widths=None):
    """airs: [(cols [columns, rows] canonical, interactions)] (tests/_bus_multiset.py); widths: the main widths where cols also holds
    preprocessed columns -> detect_rows of the active rows; raises Status(7, air << 32 | row) first"""
    rows, worst = [], None
    for a, (cols, interactions) in enumerate(airs):
        got = bridge(cols, interactions, bus) if interactions is not None else None
        if got is None:
            continue
        active, bad, pc, ts = got
        if bad.any():
            w = (a << 32) | int(np.nonzero(bad)[0][0])
            worst = w if worst is None else min(worst, w)
        width = len(cols) if widths is None else widths[a]
        cells = np.asarray(cols[:width]).astype(np.int64)
        seg = 0 if segments is None else int(segments[a])
        for r in np.nonzero(active)[0].tolist():
            rows.append((a, seg, int(ts[r]), int(pc[r]), cells[:, r].tolist()))
    if worst is not None:
        raise Status(7, worst)
    return detect_rows(rows, blocks, pc_step)


def as_dict(ec):
    """a powdr_amd.empirical.EmpiricalConstraints in the shape detect() returns"""
    return dict(column_ranges_by_pc={pc: [tuple(r) for r in v] for pc, v in ec.column_ranges_by_pc.items()},
                equivalence_classes_by_block={b: [[tuple(c) for c in cls] for cls in v] for b, v in ec.equivalence_classes_by_block.items()},
                pc_counts=dict(ec.pc_counts), air_id_by_pc=dict(ec.debug_info["air_id_by_pc"]))


def to_constraints(d, column_names=None):
    from powdr_amd import empirical

    return empirical.EmpiricalConstraints({pc: list(v) for pc, v in d["column_ranges_by_pc"].items()},
                                          {b: [list(c) for c in v] for b, v in d["equivalence_classes_by_block"].items()}, dict(d["pc_counts"]),
                                          {"air_id_by_pc": dict(d["air_id_by_pc"]), "column_names_by_air_id": dict(column_names or {})})


# ---- the block log AIR ------------------------------------------------------------------------------------------------------------------
def block_log_interactions(bus=0):
    col = lambda c: [OP_PUSH_APC, c]
    inter, spans, bc = [], [], []
    for mult in ([OP_PUSH_APC, 0, OP_NEG], col(0)):
        inter.append((bus, 2, len(spans)))
        for prog in (mult, col(1), col(2)):
            spans.append((len(bc), len(prog)))
            bc += prog
    return np.array(inter, np.uint32).reshape(-1, 3), np.array(spans, np.uint32).reshape(-1, 2), np.array(bc, np.uint32)


def block_log(rows, n_data, log_h=None, places=None):
    """rows: [(pc, ts, [data])] -> cols [3 + n_data, 2^log_h] canonical: row k at position places[k] (default k), zeros elsewhere"""
    n = len(rows)
    log_h = max(1, (max(n, 2) - 1).bit_length()) if log_h is None else log_h
    cols = np.zeros((3 + n_data, 1 << log_h), np.uint32)
    at = np.arange(n) if places is None else np.asarray(places)
    assert len(at) == n and len(set(at.tolist())) == n and (n == 0 or at.max() < 1 << log_h)
    if n:
        cols[0, at] = 1
        cols[1, at] = [r[0] for r in rows]
        cols[2, at] = [r[1] for r in rows]
        data = np.array([list(r[2]) + [0] * (n_data - len(r[2])) for r in rows], np.uint32).reshape(n, n_data)
        cols[3:, at] = data.T
    return cols
