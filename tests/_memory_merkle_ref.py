"""The numpy reference of the memory Merkle AIR's trace (powdr_amd/memory_tree.py merkle_air / merkle_trace, pw_memory_merkle_trace;
DESIGN.md §5n), a second route to it: from the records and node ids of tests/_memory_tree_ref.SparseTree.update, per node from
dictionaries — no search in a sorted array — and the pieces the tests put around it: a stand-in for the boundary AIR's leaf sends, the
Poseidon2 chip's rows for whatever pairs a trace asks for (tests/_poseidon2_air_ref), the AIR's constraints by name
(tests/_system_airs_ref.eval_constraints, the public values put in as constants) and the buses as multisets (tests/_bus_multiset).

Words are canonical; a trace is int64 [55, 2^log_height], one numpy row per column, in the order of memory_tree.MERKLE_COLUMNS."""
import numpy as np

from tests import _bus_multiset as bm
from tests import _memory_tree_ref as tree_ref
from tests import _poseidon2_air_ref as p2
from tests import _system_airs_ref as sys_ref

P = p2.P
WIDTH = 55
VALID, IS_ROOT, IS_LEAF, LEFT_TOUCHED, RIGHT_TOUCHED, LEVEL, INDEX = range(7)
LEFT0, RIGHT0, OUT0, LEFT1, RIGHT1, OUT1 = (7 + 8 * k for k in range(6))
PHASE_BIT = 1 << 63
BUS_COMPRESS, BUS_MERKLE, BUS_LEAF = 5, 8, 9


def node_of(node_id):
    node_id = int(node_id) & ~PHASE_BIT
    return node_id >> 56, node_id & ((1 << 56) - 1)


def trace(records, ids, n_rows, height, log_height=None):
    """records [25, >= n_rows] canonical, ids [n_rows] -> (cols int64 [55, 2^log_height], {(level, index): row}): one row per node,
    the root first, then by descending (level, index) — the records order backwards; log_height = the smallest height of at least 1
    that holds the nodes, unless given"""
    assert n_rows % 2 == 0 and n_rows > 0
    n = n_rows // 2
    records = np.asarray(records).astype(np.int64)
    before = {node_of(ids[j]): records[1:25, j] for j in range(n)}
    after = {node_of(ids[n + j]): records[1:25, n + j] for j in range(n)}
    assert len(before) == n and set(before) == set(after) and all(int(ids[j]) < PHASE_BIT <= int(ids[n + j]) for j in range(n))
    lh = max(1, (n - 1).bit_length())
    if log_height is not None:
        assert log_height >= lh
        lh = log_height
    cols = np.zeros((WIDTH, 1 << lh), np.int64)
    where = {}
    for r, (level, index) in enumerate(sorted(before, reverse=True)):
        where[(level, index)] = r
        cols[:7, r] = [1, (level, index) == (height, 0), level == 0, (level - 1, 2 * index) in before, (level - 1, 2 * index + 1) in before, level, index]
        cols[LEFT0:LEFT1, r] = before[(level, index)]
        cols[LEFT1:, r] = after[(level, index)]
    return cols, where


def public_of(cols):
    """root before | root after as the root row (row 0) states them"""
    return np.concatenate([cols[OUT0:OUT0 + 8, 0], cols[OUT1:OUT1 + 8, 0]]).astype(np.int64)


def leaf_sender(keys, init, fin, bus=BUS_LEAF, min_log_h=1):
    """The boundary AIR's leaf sends without a boundary AIR: columns [is_valid, key, init0..3, fin0..3], one interaction that sends
    (key, init0..3, fin0..3) is_valid times on `bus`. init / fin: [n, >= 4] words. -> (cols int64 [10, 2^k], interactions)"""
    from powdr_amd import periphery

    n = len(keys)
    lh = max(min_log_h, 1, (n - 1).bit_length() if n else 0)
    cols = np.zeros((10, 1 << lh), np.int64)
    cols[0, :n], cols[1, :n] = 1, np.asarray(keys, dtype=np.int64)
    cols[2:6, :n] = np.asarray(init, dtype=np.int64).reshape(n, -1)[:, :4].T
    cols[6:10, :n] = np.asarray(fin, dtype=np.int64).reshape(n, -1)[:, :4].T
    return cols, periphery._tables(bus, [(periphery._col(0), [periphery._col(1 + j) for j in range(9)])])


def chip(cols, constants, bus=BUS_COMPRESS):
    """The Poseidon2 chip for the pairs the valid rows of a Merkle trace send, in witness order (interaction, row): every pair gets the
    row of its TRUE digest, as pw_poseidon2_compress_trace gives it — a row that states another digest leaves the bus open.
    -> (cells int64 [307, 2^k], interactions)"""
    from powdr_amd import periphery

    on = np.nonzero(cols[VALID])[0].tolist()
    requests = [(cols[first:first + 16, r].tolist(), int(cols[VALID, r])) for first in (LEFT0, LEFT1) for r in on]
    cells, _ = p2.compress_rows(requests, constants)
    col = periphery._col
    return cells.astype(np.int64), periphery._tables(bus, [(periphery._neg_col(0), [col(p2.IN + i) for i in range(16)] + [col(p2.OUT + j) for j in range(8)])])


def violations(air, names, cols, public):
    """{constraint name: rows where it does not vanish} of a SystemAir with public values on canonical columns: the public operands
    (prover.RowOperands.public(k)) are put into the programs as constants, then tests/_system_airs_ref.eval_constraints"""
    from types import SimpleNamespace

    bound = 2 * air.width + 3
    bc = np.asarray(air.cons[0]).astype(np.int64).copy()
    i = 0
    while i < len(bc):
        if bc[i] == 0 and bc[i + 1] >= bound:
            bc[i], bc[i + 1] = 1, int(public[bc[i + 1] - bound]) % P
        i += 2 if bc[i] in (0, 1) else 1
    assert len(names) == len(np.asarray(air.cons[1]).reshape(-1, 2))
    return {names[k]: rows for k, rows in sys_ref.eval_constraints(SimpleNamespace(cons=(bc, air.cons[1])), list(cols))}


def unbalanced(airs, buses=(BUS_COMPRESS, BUS_MERKLE, BUS_LEAF)):
    """the buses of `buses` on which some tuple's multiplicities do not cancel: airs = [(cols, interactions)] as for _bus_multiset.tally"""
    table, _ = bm.tally(airs)
    return {key[0] for key, e in table.items() if e[0] and key[0] in buses}


def row_tuples(cols, r, interactions):
    """the signed multiset of bus tuples row r alone contributes: {(bus, n_args, args): net multiplicity}, zeros dropped"""
    table, _ = bm.tally([([c[r:r + 1] for c in cols], interactions)])
    return {key: e[0] for key, e in table.items() if e[0]}


def rehash_up(cols, where, node, phase, constants):
    """The adversary's repair after changing a child word of `node` in one phase: out of that phase is hashed again on the node's row
    and handed to its parent's row as the left or right child, up to the root -> the new root [8]"""
    left, out = (LEFT0, OUT0) if phase == 0 else (LEFT1, OUT1)
    level, index = node
    while True:
        r = where[(level, index)]
        digest = tree_ref.compress(cols[left:left + 16, r][None], constants)[0].astype(np.int64)
        cols[out:out + 8, r] = digest
        if (level + 1, index >> 1) not in where:
            return digest
        side = left + 8 * (index & 1)
        cols[side:side + 8, where[(level + 1, index >> 1)]] = digest
        level, index = level + 1, index >> 1
