"""The numpy reference of the bus mock prover (pw_check_segment_buses): the multiset of bus tuples of a segment.

An AIR is (cols, interactions): cols = the canonical cells the interaction programs read, shape [columns, rows] (main columns, then
the preprocessed ones), interactions = (inter[n x 3] = {bus, n_args, first span}, spans[m x 2] = {off, len} laid out
[mult, arg0, arg1, ...], post-fix bytecode with column-index operands) — what prover.Prover takes. The programs are evaluated by
oracle.original_chips.eval_postfix; a tuple is (bus, n_args, args): (a, b) and (a, b, 0) are different tuples."""
import numpy as np

from oracle import original_chips as ooc

P = ooc.P


def tally(airs):
    """-> ({(bus, n_args, args): [sum of multiplicities mod p, smallest (air, interaction, row), contributions]}, {bus: active triples})"""
    table, active = {}, {}
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
            bus %= P
            active.setdefault(bus, 0)
            m = value(first)
            on = np.nonzero(m)[0]
            if not len(on):
                continue
            args = np.stack([value(first + 1 + j)[on] for j in range(n_args)], axis=1) if n_args else np.zeros((len(on), 0), np.int64)
            active[bus] += len(on)
            for r, mult, tup in zip(on.tolist(), m[on].tolist(), args.tolist()):
                e = table.setdefault((bus, n_args, tuple(tup)), [0, (a, i, r), 0])
                e[0] = (e[0] + mult) % P
                e[1] = min(e[1], (a, i, r))
                e[2] += 1
    return table, active


def expected(airs, buses=None, tally_all=False):
    """What check_segment_buses reports without overflow and with a tuple_cap above the count: (summaries, tuples) as lists of dicts."""
    table, active = tally(airs)
    ids = sorted(active) if buses is None else sorted(set(int(b) % P for b in buses))
    unbalanced = {b: [] for b in ids}
    for key in sorted(k for k, e in table.items() if e[0] and k[0] in unbalanced):
        unbalanced[key[0]].append(key)
    summaries = [dict(bus=b, status=1 if unbalanced[b] else 0, n_active=active.get(b, 0), n_unbalanced=len(unbalanced[b])) for b in ids]
    tuples = []
    for b in ids:
        for key in unbalanced[b]:
            e = table[key]
            tuples.append(dict(bus=b, n_args=key[1], args=list(key[2][:16]), net_multiplicity=e[0], air=e[1][0], interaction=e[1][1],
                               row=e[1][2], n_contributions=e[2]))
    return summaries, tuples


def verdicts(airs):
    """{bus: (active triples, balanced)} without the per-tuple dict: the tuples are hashed to 64 bits (wrapping multiply-xor over
    n_args and the arguments), the centred multiplicities added per hash by sort + reduceat. For AIRs too large for tally()'s Python
    loop; a hash collision between two of N tuples has probability about N^2 / 2^65."""
    keys, mults, active = {}, {}, {}
    c0, c1 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F)
    for cols, interactions in airs:
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

        for bus, n_args, first in inter.tolist():
            bus %= P
            active.setdefault(bus, 0)
            m = value(first)
            on = np.nonzero(m)[0]
            if not len(on):
                continue
            active[bus] += len(on)
            k = np.full(len(on), n_args + 1, np.uint64) * c0
            for j in range(n_args):
                k = (k ^ value(first + 1 + j)[on].astype(np.uint64)) * c1 + c0
            keys.setdefault(bus, []).append(k)
            mm = m[on]
            mults.setdefault(bus, []).append(np.where(mm > P // 2, mm - P, mm))
    out = {}
    for bus, n in active.items():
        balanced = True
        if n:
            k, mm = np.concatenate(keys[bus]), np.concatenate(mults[bus])
            order = np.argsort(k, kind="stable")
            k, mm = k[order], mm[order]
            starts = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
            balanced = not (np.add.reduceat(mm, starts) % P).any()
        out[bus] = (n, balanced)
    return out
