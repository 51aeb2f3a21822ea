"""TEST INFRASTRUCTURE — the second route to the metered cut of an execution, written from the definition as a
sequential walk over Python lists: a running set of keys and a running set of (level, key >> level), grown position by position —
no table, no sort, no prefix array. Positions, classes and allowed cuts are tests/_execution_segments_ref.py's; the accesses come
from oracle.original_chips.eval_postfix, as tests/_execution_states_ref.py takes its registers.

The definition. An access is an active interaction (non-zero multiplicity) on the memory bus, with the 7 arguments (as, ptr, d0..d3,
t), of the row at a position; its key is (as - 1) * 2^29 + ptr; as not in {1, 2}, ptr >= 2^29 or key >= 2^H is status 15 with the
smallest packed (air, interaction, row). For a window [p, q): B = the distinct keys of its accesses, M = the distinct (l, key >> l),
l = 0 .. H, P = 2 M (an upper bound on the Poseidon2 chip's rows, not a count). fits_sys(p, q) = fits(p, q), B <= 2^cap[0],
M <= 2^cap[1], P <= 2^cap[2], and under max_cells the cell sum with width[k] * padded_sys(count_k) added for every width[k] > 0;
padded_sys(0) = 0, else max(2, padded(n)). b_(s+1) = the largest allowed q with fits_sys(b_s, q); status 13 at b_s where there is
none, status 14 as in §5v."""
from collections import Counter

import numpy as np

from oracle import original_chips as ooc
from tests import _apc_sources_ref as aref
from tests import _execution_segments_ref as ref
from tests import _execution_states_ref as sref

P = ooc.P
Status = ref.Status
PAD = ref.PAD
WIDTHS = (18, 55, 307)  # boundary, memory Merkle, Poseidon2


def padded_sys(n, min_log_height=0):
    return 0 if n == 0 else max(2, ref.padded(n, min_log_height))


def key_of(space, ptr, height):
    """the key of (as, ptr) in a tree of `height`, or None"""
    if space not in (1, 2) or ptr >= 1 << 29:
        return None
    key = (space - 1) * (1 << 29) + ptr
    return key if key < 1 << height else None


def accesses(airs, pos, part, memory_bus, height):
    """pos: [(air, row)] per position, part: the AIRs on the bridge -> the keys of every position's accesses (a list per position);
    raises Status 15 with the smallest witness of an access without a key"""
    at = {ar: p for p, ar in enumerate(pos)}
    out, bad = [[] for _ in pos], []
    for a, (cols, interactions) in enumerate(airs):
        if interactions is None or a not in part:
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
            on = np.nonzero(value(first) != 0)[0]
            space, ptr = value(first + 1), value(first + 2)
            for r in on.tolist():
                if (a, r) not in at:
                    continue
                key = key_of(int(space[r]), int(ptr[r]), height)
                if key is None:
                    bad.append((a, i, r))
                else:
                    out[at[(a, r)]].append(key)
    if bad:
        raise Status(15, sref.pack_witness(*min(bad)))
    return out


def counts(keys_at, p, q, height):
    """the definition itself: (B, M, P) of the window [p, q)"""
    keys = {k for ks in keys_at[p:q] for k in ks}
    nodes = {(level, k >> level) for k in keys for level in range(height + 1)}
    return len(keys), len(nodes), 2 * len(nodes)


def merkle_closed_form(keys, height):
    """M of a set of keys: H + 1 + sum bitlen(k_(j-1) xor k_j) over the sorted distinct keys (0 for none)"""
    ks = sorted(set(keys))
    return (height + 1 + sum((a ^ b).bit_length() for a, b in zip(ks, ks[1:]))) if ks else 0


def fits_sys(cls, keys_at, width, p, q, max_log_height, height, caps, sys_widths=WIDTHS, min_log_height=0, max_cells=0):
    """the definition itself: counts over [p, q)"""
    cnt = Counter(c for c in cls[p:q] if c is not None)
    if any(n > 1 << max_log_height for n in cnt.values()):
        return False
    sys = counts(keys_at, p, q, height)
    if any(n > 1 << cap for n, cap in zip(sys, caps)):
        return False
    if not max_cells:
        return True
    cells = sum(width[c] * ref.padded(n, min_log_height) for c, n in cnt.items())
    cells += sum(w * padded_sys(n, min_log_height) for w, n in zip(sys_widths, sys) if w)
    return cells <= max_cells


def cut(cls, ok, keys_at, width, max_log_height, height, caps, sys_widths=WIDTHS, min_log_height=0, max_cells=0, max_segments=0):
    """the walk: position by position with running counts and running sets -> (bounds, [(B, M, P)] per segment, how often the
    largest q that fits was not allowed)"""
    n, cap, top = len(cls), 1 << max_log_height, max_segments or 1 << 20
    bounds, heights, snapped, b = [0], [], 0, 0
    while b < n:
        if len(bounds) - 1 == top:
            raise Status(14, b)
        cnt, cells, best, last, at_best = Counter(), 0, None, b, None
        keys, nodes = set(), set()
        for q in range(b + 1, n + 1):
            c = cls[q - 1]
            if c is not None:
                cells += width[c] * (ref.padded(cnt[c] + 1, min_log_height) - ref.padded(cnt[c], min_log_height))
                cnt[c] += 1
                if cnt[c] > cap:
                    break
            for k in keys_at[q - 1]:
                if k not in keys:
                    keys.add(k)
                    for level in range(height + 1):
                        nodes.add((level, k >> level))
            sys = (len(keys), len(nodes), 2 * len(nodes))
            if any(x > 1 << c for x, c in zip(sys, caps)):
                break
            if max_cells and cells + sum(w * padded_sys(x, min_log_height) for w, x in zip(sys_widths, sys) if w) > max_cells:
                break
            last = q
            if ok[q]:
                best, at_best = q, sys
        if best is None:
            raise Status(13, b)
        snapped += not ok[last]
        bounds.append(best)
        heights.append(at_best)
        b = best
    return bounds, heights, snapped


def fewest_segments(cls, ok, keys_at, width, max_log_height, height, caps, sys_widths=WIDTHS, min_log_height=0, max_cells=0):
    """brute force over every set of allowed cuts (small inputs): the fewest segments of a valid cut, None if there is none"""
    n = len(cls)
    inner = [q for q in range(1, n) if ok[q]]
    best = None
    for mask in range(1 << len(inner)):
        b = [0] + [q for i, q in enumerate(inner) if mask >> i & 1] + [n]
        if best is not None and len(b) - 1 >= best:
            continue
        if all(fits_sys(cls, keys_at, width, p, q, max_log_height, height, caps, sys_widths, min_log_height, max_cells) for p, q in zip(b, b[1:])):
            best = len(b) - 1
    return best


def segments(airs, final_pc, max_log_height, height=30, caps=None, sys_widths=WIDTHS, memory_bus=1, calls=(), apc_widths=(), min_log_height=0, max_cells=0,
             max_segments=0, segment_numbers=None, bus=0):
    """tests/_execution_segments_ref.segments with the meter: the same dict and system_heights [(B, M, P)]; raises Status 7, 4, 11,
    15, 13, 14. caps: None = max_log_height for all three, an int, or (b, m, p)."""
    caps = (max_log_height,) * 3 if caps is None else (caps,) * 3 if isinstance(caps, int) else tuple(caps)
    calls = [tuple(c) for c in calls]
    pos, part = aref.where(airs, segment_numbers, bus)
    _, pcs, keys = sref.positions(airs, final_pc, segment_numbers, bus)
    n = len(pos)
    late = [j for j, (_, _, to) in enumerate(calls) if to > n]
    if late:
        raise Status(11, late[0])
    keys_at = accesses(airs, pos, set(part), memory_bus, height)
    cls = ref.classes([a for a, _ in pos], calls)
    width = {a: len(cols) for a, (cols, _) in enumerate(airs)}
    width.update({("apc", a): w for a, w in enumerate(apc_widths)})
    if not max_cells:
        width.update({c: 0 for c in cls if c is not None and c not in width})
    bounds, sys_heights, snapped = cut(cls, ref.allowed(n, calls), keys_at, width, max_log_height, height, caps, sys_widths, min_log_height, max_cells, max_segments)
    heights, lists, first_call = [], {}, []
    for s, (p, q) in enumerate(zip(bounds, bounds[1:])):
        heights.append(dict(Counter(c for c in cls[p:q] if c is not None)))
        by_air = {}
        for i in range(p, q):
            by_air.setdefault(pos[i][0], []).append(pos[i][1])
        for a, rows in by_air.items():
            lists[(s, a)] = rows + [PAD] * (ref.padded(len(rows), min_log_height) - len(rows))
    for b in bounds:
        first_call.append(sum(1 for _, start, _ in calls if start < b))
    return dict(positions=n, bounds=bounds, starts=[(pcs[b], keys[b]) for b in bounds[:-1]], final_pc=pcs[n], first_call=first_call, heights=heights, lists=lists,
                snapped=snapped, system_heights=[tuple(h) for h in sys_heights], accesses=sum(len(k) for k in keys_at))
