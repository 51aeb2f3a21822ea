"""TEST INFRASTRUCTURE — the second route to the cut of an execution into segments, written from the definition as a
sequential walk over Python lists: no sorting by class, no lower bounds, no bisection.

The definition. Position i < N is the active row with the i-th smallest time key, in AIR air(i). Calls are (apc_id, from, to),
ascending and non-overlapping. A position covered by call j has the class ("apc", apc_id) if it is from_j and no class otherwise; an
uncovered position has the class air(i). cnt_c(p, q) = the positions of class c in [p, q). padded(n) = 0 for n == 0, else
max(2^min_log_height, next power of two >= n). fits(p, q): every cnt_c(p, q) <= 2^max_log_height, and max_cells == 0 or
sum_c width_c * padded(cnt_c(p, q)) <= max_cells. allowed(q): no call has from < q < to. b_0 = 0, b_(s+1) = the largest allowed q in
(b_s, N] with fits(b_s, q); status 14 at the position reached when max_segments (0 = 2^20) segments do not reach N, status 13 at b_s
when no allowed q fits."""
from collections import Counter

from tests import _apc_sources_ref as aref
from tests import _empirical_ref as eref
from tests import _execution_states_ref as sref

Status = eref.Status
PAD = 0xFFFFFFFF


def padded(n, min_log_height=0):
    if n == 0:
        return 0
    p = 1
    while p < n:
        p *= 2
    return max(1 << min_log_height, p)


def classes(air_of, calls):
    """the class of every position (None: covered, not a call's first position)"""
    out = list(air_of)
    for a, start, end in calls:
        for p in range(start, end):
            out[p] = None
        out[start] = ("apc", a)
    return out


def allowed(n, calls):
    ok = [True] * (n + 1)
    for _, start, end in calls:
        for q in range(start + 1, end):
            ok[q] = False
    return ok


def fits(cls, width, p, q, max_log_height, min_log_height=0, max_cells=0):
    """the definition itself: a count over [p, q)"""
    cnt = Counter(c for c in cls[p:q] if c is not None)
    if any(n > 1 << max_log_height for n in cnt.values()):
        return False
    return max_cells == 0 or sum(width[c] * padded(n, min_log_height) for c, n in cnt.items()) <= max_cells


def cut(cls, ok, width, max_log_height, min_log_height=0, max_cells=0, max_segments=0):
    """the walk: position by position with running counts -> (bounds, how often the largest q that fits was not allowed)"""
    n, cap, top = len(cls), 1 << max_log_height, max_segments or 1 << 20
    bounds, snapped, b = [0], 0, 0
    while b < n:
        if len(bounds) - 1 == top:
            raise Status(14, b)
        cnt, cells, best, last = Counter(), 0, None, b
        for q in range(b + 1, n + 1):
            c = cls[q - 1]
            if c is not None:
                cells += width[c] * (padded(cnt[c] + 1, min_log_height) - padded(cnt[c], min_log_height))
                cnt[c] += 1
                if cnt[c] > cap or (max_cells and cells > max_cells):
                    break
            last = q
            if ok[q]:
                best = q
        if best is None:
            raise Status(13, b)
        snapped += not ok[last]
        bounds.append(best)
        b = best
    return bounds, snapped


def fewest_segments(cls, ok, width, max_log_height, min_log_height=0, max_cells=0):
    """brute force over every set of allowed cuts (small inputs): the fewest segments of a valid cut, None if there is none"""
    n = len(cls)
    inner = [q for q in range(1, n) if ok[q]]
    best = None
    for mask in range(1 << len(inner)):
        b = [0] + [q for i, q in enumerate(inner) if mask >> i & 1] + [n]
        if best is not None and len(b) - 1 >= best:
            continue
        if all(fits(cls, width, p, q, max_log_height, min_log_height, max_cells) for p, q in zip(b, b[1:])):
            best = len(b) - 1
    return best


def segments(airs, final_pc, max_log_height, calls=(), apc_widths=(), min_log_height=0, max_cells=0, max_segments=0, segment_numbers=None, bus=0):
    """airs: [(cols [columns, rows], interactions)] on the host -> dict(positions, bounds, starts [(pc, time key)], final_pc, first_call,
    heights [{class: rows}], lists {(segment, air): [rows .. padded with PAD]}, snapped); raises Status 7, 4, 11, 13, 14"""
    calls = [tuple(c) for c in calls]
    pos, _ = aref.where(airs, segment_numbers, bus)
    _, pcs, keys = sref.positions(airs, final_pc, segment_numbers, bus)
    n = len(pos)
    late = [j for j, (_, _, to) in enumerate(calls) if to > n]
    if late:
        raise Status(11, late[0])
    cls = classes([a for a, _ in pos], calls)
    width = {a: len(cols) for a, (cols, _) in enumerate(airs)}
    width.update({("apc", a): w for a, w in enumerate(apc_widths)})
    if not max_cells:
        width.update({c: 0 for c in cls if c is not None and c not in width})
    bounds, snapped = cut(cls, allowed(n, calls), width, max_log_height, min_log_height, max_cells, max_segments)
    heights, lists, first_call = [], {}, []
    for s, (p, q) in enumerate(zip(bounds, bounds[1:])):
        heights.append(dict(Counter(c for c in cls[p:q] if c is not None)))
        by_air = {}
        for i in range(p, q):
            by_air.setdefault(pos[i][0], []).append(pos[i][1])
        for a, rows in by_air.items():
            lists[(s, a)] = rows + [PAD] * (padded(len(rows), min_log_height) - len(rows))
    for b in bounds:
        first_call.append(sum(1 for _, start, _ in calls if start < b))
    return dict(positions=n, bounds=bounds, starts=[(pcs[b], keys[b]) for b in bounds[:-1]], final_pc=pcs[n], first_call=first_call, heights=heights, lists=lists,
                snapped=snapped)
