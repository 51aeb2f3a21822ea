"""TEST INFRASTRUCTURE — the second route to the APC traces of direct mode, numpy only: the index lists from
tests/_apc_sources_ref.py `where`, and the definition written as indexing.

The definition. With positions, layout (air_a[k], occ_a[k]) and rbs_a[A] as in tests/_apc_sources_ref.py, the index list of (a, A) has
n_calls(a) * rbs entries: L[j * rbs + occ_a[k]] = row(from_j + k) for every k with air_a[k] == A. A job (apc, cells, out_height,
out_width) with cells (instr, col, apc_col) gives the column-major matrix with
    out[apc_col, r] = trace_A[col, L[r * rbs + occ]] for r < n_calls(apc), 0 for n_calls(apc) <= r < out_height,   (A, occ) = layout[instr]
and every column no cell names left as it was. `from_sources` is the `_apc_tracegen` definition of include/powdr_gpu.h on the source
matrices of tests/_apc_sources_ref.py `apply` with Subst {A, col, occ, apc_col}: the two must agree word for word."""
import numpy as np

from tests import _apc_sources_ref as ref

FILL = 0xA5A5A5A5


def lists(airs, cycle_counts, calls, segments=None, bus=0):
    """-> (layout [(n_calls, [(air, occ)])] per APC, {(apc, air): (L u32[n_calls * rbs], rbs)}); the statuses are `ref.apply`'s"""
    pos, _ = ref.where(airs, segments, bus)
    by_apc = {}
    for a, start, end in calls:
        assert end - start == cycle_counts[a] and end <= len(pos)
        by_apc.setdefault(a, []).append(start)
    layout, out = [], {}
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
            L = np.full(len(starts) * rbs, 0xFFFFFFFF, np.uint32)
            for j, s in enumerate(starts):
                for k in range(length):
                    if air_of[k] == A:
                        assert pos[s + k][0] == A
                        L[j * rbs + occ[k]] = pos[s + k][1]
            assert (L != 0xFFFFFFFF).all()
            out[(a, A)] = (L, rbs)
    return layout, out


def traces(airs, layout, index_lists, apc, cells, out_height, out_width, fill=FILL):
    """the definition -> u32 [out_width, out_height]; columns no cell names hold `fill`"""
    n_calls, instructions = layout[apc]
    assert out_height >= n_calls
    out = np.full((out_width, out_height), fill, np.uint32)
    for instr, col, apc_col in cells:
        out[apc_col] = 0
        if n_calls:
            A, occ = instructions[instr]
            L, rbs = index_lists[(apc, A)]
            out[apc_col, :n_calls] = np.asarray(airs[A][0])[col, L[np.arange(n_calls) * rbs + occ]]
    return out


def from_sources(sources, layout, apc, cells, out_height, out_width, fill=FILL):
    """_apc_tracegen on `ref.apply(...)["sources"]`: out[apc_col, r] = r < n_calls ? S_A[col, occ + r * rbs] : 0"""
    n_calls, instructions = layout[apc]
    out = np.full((out_width, out_height), fill, np.uint32)
    for instr, col, apc_col in cells:
        out[apc_col] = 0
        if n_calls:
            A, occ = instructions[instr]
            m, rbs = sources[(apc, A)]
            out[apc_col, :n_calls] = m[col, occ + np.arange(n_calls) * rbs]
    return out


def all_cells(layout, apc, widths):
    """every cell of every instruction of the APC, one APC column each: [(instr, col, apc_col)]"""
    cells = [(i, col) for i, (air, _) in enumerate(layout[apc][1]) for col in range(widths[air])]
    return [(i, col, c) for c, (i, col) in enumerate(cells)]
