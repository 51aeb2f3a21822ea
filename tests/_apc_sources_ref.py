"""TEST INFRASTRUCTURE — the second route to the source and residual traces of applied APC calls, numpy only: positions
from tests/_execution_states_ref.py `positions` (the trace route's own restatement), then the definition written as indexing.

The definition. Position i < N is the active row with the i-th smallest time key, (air(i), row(i)) where it lies. Calls are
(apc_id, from, to), ascending and non-overlapping, to - from = the APC's cycle count. For APC a with calls c_0 .. c_(n-1):
air_a[k] = air(from_0 + k), the same for every call or status 12 with the smallest position that differs from the first call's;
occ_a[k] = how many earlier instructions of a lie in the same AIR; rbs_a[A] = how many instructions of a lie in A. The source of
(a, A) has A's width and max(2^min_log_height, next power of two >= n * rbs) rows: row j * rbs + occ_a[k] is row(from_j + k) of A's
trace, every other row zero. The residual of an AIR that has the bridge: its active rows at no covered position, in row order, padded
with zero rows to max(2^min_log_height, next power of two >= their number). A call with to > N: status 11 with its index."""
import numpy as np

from tests import _empirical_ref as eref
from tests import _execution_states_ref as sref

Status = eref.Status


def pow2_at_least(n, min_log_height=0):
    return max(1 << min_log_height, 1 << max(int(n) - 1, 0).bit_length())


def where(airs, segments=None, bus=0):
    """-> ([(air, row)] per position, the AIRs that have the bridge); raises Status 7, then 4"""
    ts, _, _ = sref.positions(airs, 0, segments, bus)
    at, part = {}, []
    for a, (cols, interactions) in enumerate(airs):
        got = eref.bridge(cols, interactions, bus) if interactions is not None else None
        if got is None:
            continue
        part.append(a)
        active, _, _, t = got
        for r in np.nonzero(active)[0].tolist():
            at[int(t[r])] = (a, r)
    return [at[t] for t in ts], part


def apply(airs, cycle_counts, calls, min_log_height=0, segments=None, bus=0):
    """airs: [(cols [columns, rows], interactions)]; calls: [(apc_id, from, to)] -> dict(layout=[(n_calls, [(air, occ)])] per APC,
    sources={(apc, air): (matrix [columns, H], rbs)}, residuals={air: (matrix [columns, H], rows kept)}, positions=N)"""
    pos, part = where(airs, segments, bus)
    n = len(pos)
    late = [j for j, (_, _, to) in enumerate(calls) if to > n]
    if late:
        raise Status(11, late[0])
    by_apc = {}
    for a, start, end in calls:
        assert end - start == cycle_counts[a]
        by_apc.setdefault(a, []).append(start)
    wrong = []
    for a, starts in by_apc.items():
        first = [pos[starts[0] + k][0] for k in range(cycle_counts[a])]
        wrong += [s + k for s in starts[1:] for k in range(cycle_counts[a]) if pos[s + k][0] != first[k]]
    if wrong:
        raise Status(12, min(wrong))
    layout, sources = [], {}
    covered = set()
    for a, length in enumerate(cycle_counts):
        starts = by_apc.get(a, [])
        if not starts:
            layout.append((0, []))
            continue
        air_of = [pos[starts[0] + k][0] for k in range(length)]
        occ = [air_of[:k].count(air_of[k]) for k in range(length)]
        layout.append((len(starts), list(zip(air_of, occ))))
        for A in sorted(set(air_of)):
            rbs = air_of.count(A)
            cols = np.asarray(airs[A][0])
            m = np.zeros((cols.shape[0], pow2_at_least(len(starts) * rbs, min_log_height)), cols.dtype)
            for j, s in enumerate(starts):
                for k in range(length):
                    if air_of[k] == A:
                        m[:, j * rbs + occ[k]] = cols[:, pos[s + k][1]]
            sources[(a, A)] = (m, rbs)
        covered |= {pos[s + k] for s in starts for k in range(length)}
    residuals = {}
    for A in part:
        cols = np.asarray(airs[A][0])
        keep = sorted(r for (a, r) in pos if a == A and (a, r) not in covered)
        m = np.zeros((cols.shape[0], pow2_at_least(len(keep), min_log_height)), cols.dtype)
        m[:, :len(keep)] = cols[:, keep]
        residuals[A] = (m, len(keep))
    return dict(layout=layout, sources=sources, residuals=residuals, positions=n)
