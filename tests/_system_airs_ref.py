"""The numpy reference of the three system AIRs' traces, two ways: from the ground truth of a chained execution
(tests/_chained_vm.Execution: what every location held before and after, where the execution began and ended, how often every
instruction ran) and, independently of any executor, from what tests/_bus_multiset.tally leaves over on the three buses. Canonical
words, one numpy row per column, in the column order of powdr_amd.system_airs."""
import numpy as np

from oracle import original_chips as ooc

P = ooc.P
BOUNDARY_WIDTH = 18
NO_CONS = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))


def boundary_from_arrays(space, ptr, init_bytes, init_ts, fin_bytes, fin_ts, min_log_h=1):
    """one entry per location, in any order (bytes: [4, n]) -> u32[18, 2^k], k = ceil(log2 n) (at least min_log_h): rows sorted by
    (as, ptr), [is_valid, as, ptr, p_lo, p_hi, init bytes, init_ts, fin bytes, fin_ts, same_as, d_lo, d_hi]"""
    space, ptr = np.asarray(space, np.int64), np.asarray(ptr, np.int64)
    n = len(space)
    order = np.lexsort((ptr, space))
    space, ptr = space[order], ptr[order]
    assert n < 2 or ((space[1:] > space[:-1]) | (ptr[1:] > ptr[:-1])).all(), "an address occurs twice"
    lh = max(min_log_h, 1, (n - 1).bit_length() if n else 0)
    t = np.zeros((BOUNDARY_WIDTH, 1 << lh), np.int64)
    t[0, :n], t[1, :n], t[2, :n], t[3, :n], t[4, :n] = 1, space, ptr, ptr & 0x1FFFF, ptr >> 17
    t[5:9, :n], t[9, :n] = np.asarray(init_bytes, np.int64)[:, order], np.asarray(init_ts, np.int64)[order]
    t[10:14, :n], t[14, :n] = np.asarray(fin_bytes, np.int64)[:, order], np.asarray(fin_ts, np.int64)[order]
    if n > 1:
        same = space[1:] == space[:-1]
        d = np.where(same, ptr[1:] - ptr[:-1] - 1, 0)
        t[15, :n - 1], t[16, :n - 1], t[17, :n - 1] = same, d & 0x1FFFF, d >> 17
    return t.astype(np.uint32)


def boundary_trace(initial, final, min_log_h=1):
    """initial / final: {(as, ptr): (word, timestamp)} over the same locations -> boundary_from_arrays of them"""
    assert set(initial) == set(final)
    keys = sorted(initial)
    by = lambda d: (np.array([[(d[k][0] >> (8 * i)) & 0xFF for k in keys] for i in range(4)], np.int64).reshape(4, len(keys)),
                    np.array([d[k][1] for k in keys], np.int64))
    (b0, t0), (b1, t1) = by(initial), by(final)
    return boundary_from_arrays([k[0] for k in keys], [k[1] for k in keys], b0, t0, b1, t1, min_log_h)


def connector_trace(start, end):
    """start / end: (pc, timestamp) -> u32[2, 2]: columns pc, timestamp; row 0 the initial state, row 1 the final one"""
    return np.array([[start[0], end[0]], [start[1], end[1]]], np.uint32)


def program_freq(table, counts):
    """table u32[9, rows]; counts {pc: times executed} -> u32[1, rows]"""
    freq = np.zeros((1, table.shape[1]), np.uint32)
    pcs = table[0].tolist()
    for pc, n in counts.items():
        freq[0, pcs.index(pc)] = n % P
    return freq


def _word(b):
    assert all(0 <= x < 256 for x in b)
    return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24)


def from_leftovers(tally_table, program_table, buses=(0, 1, 2)):
    """The three traces from the tuples the SENDERS of a segment leave unbalanced (tally_table: the first result of
    tests/_bus_multiset.tally over the instruction AIRs alone): on the memory bus the tuples received once more than sent are the
    initial values and those sent once more than received the final ones; on the execution bridge one of each; on the PC lookup
    every tuple is a program row, sent as often as it ran."""
    b_exec, b_mem, b_pc = buses
    initial, final, start, end, counts = {}, {}, [], [], {}
    for (bus, n_args, args), (net, _, _) in tally_table.items():
        if not net:
            continue
        if bus == b_mem:
            assert n_args == 7 and net in (1, P - 1), (args, net)
            into = final if net == 1 else initial
            assert (args[0], args[1]) not in into, "two leftovers at one address: not a consistent execution"
            into[(args[0], args[1])] = (_word(args[2:6]), args[6])
        elif bus == b_exec:
            assert n_args == 2 and net in (1, P - 1), (args, net)
            (end if net == 1 else start).append(tuple(args))
        elif bus == b_pc:
            assert n_args == 9 and net <= P // 2
            row = program_table[0].tolist().index(args[0])
            assert program_table[:, row].tolist() == list(args), "an executed instruction that is no program row"
            counts[args[0]] = net
    assert len(start) == 1 and len(end) == 1
    return program_freq(program_table, counts), connector_trace(start[0], end[0]), boundary_trace(initial, final)


def periphery_airs(tally_table, var_bus=3, bitwise_bus=6, tuple_bus=7, max_bits=17, tuple_sizes=(256, 2048)):
    """The three periphery AIRs (main layout: [tuple columns, multiplicities]) that receive every lookup the tally holds, as
    (cols, interactions) pairs for tests/_bus_multiset.tally"""
    from oracle import apc_model as om
    from powdr_amd import periphery

    var = np.zeros(1 << (max_bits + 1), np.int64)
    tup = np.zeros(tuple_sizes[0] * tuple_sizes[1], np.int64)
    bit = np.zeros(2 * 65536, np.int64)
    for (bus, n_args, args), (net, _, _) in tally_table.items():
        if bus == var_bus:
            assert n_args == 2 and args[0] < 1 << args[1] and args[1] <= max_bits, args
            var[(1 << args[1]) + args[0] - 1] += net
        elif bus == tuple_bus:
            assert n_args == 2 and args[0] < tuple_sizes[0] and args[1] < tuple_sizes[1], args
            tup[args[0] * tuple_sizes[1] + args[1]] += net
        elif bus == bitwise_bus:
            assert n_args == 4 and args[0] < 256 and args[1] < 256 and args[3] in (0, 1) and args[2] == (args[0] ^ args[1]) * args[3], args
            bit[65536 * args[3] + args[0] * 256 + args[1]] += net
    return [(om.var_range_trace(var % P), periphery.var_range_interactions(var_bus)),
            (om.tuple2_trace(tup % P, *tuple_sizes), periphery.tuple2_interactions(tuple_bus)),
            (om.bitwise_trace(bit % P), periphery.bitwise_interactions(bitwise_bus))]


def eval_constraints(air, cols):
    """Every constraint of a system AIR (powdr_amd.system_airs.SystemAir) on canonical columns [width (+ pre_width), rows], with the
    row layout of prover.RowOperands: current row, next row (cyclic), is_first_row, is_last_row, is_transition.
    -> [(constraint index, rows where it does not vanish)] for the constraints that fail"""
    cols = [np.asarray(c).astype(np.int64) for c in cols]
    rows = len(cols[0])
    r = np.arange(rows)
    operands = cols + [np.roll(c, -1) for c in cols] + [(r == 0).astype(np.int64), (r == rows - 1).astype(np.int64), (r != rows - 1).astype(np.int64)]
    bc, spans = air.cons
    bad = []
    for k, (off, ln) in enumerate(np.asarray(spans).reshape(-1, 2).tolist()):
        v = np.broadcast_to(np.asarray(ooc.eval_postfix(np.asarray(bc)[off:off + ln], operands)) % P, (rows,))
        if v.any():
            bad.append((k, np.nonzero(v)[0].tolist()))
    return bad


# ---- the synthetic "memory log" AIR: consistent memory of any size without an executor ----------------------------------------------
MEMORY_LOG_COLUMNS = ["as", "ptr"] + [f"prev{i}" for i in range(4)] + ["prev_ts"] + [f"new{i}" for i in range(4)] + ["ts", "is_valid"]


def memory_log_interactions(bus=1):
    """receive (as, ptr, prev0..3, prev_ts) and send (as, ptr, new0..3, ts), both is_valid times"""
    from powdr_amd import periphery

    col = periphery._col
    return periphery._tables(bus, [(periphery._neg_col(12), [col(0), col(1)] + [col(2 + i) for i in range(4)] + [col(6)]),
                                   (col(12), [col(0), col(1)] + [col(7 + i) for i in range(4)] + [col(11)])])


def memory_log(log_rows, n_locations, seed=0, invalid=5):
    """2^log_rows rows of which the last `invalid` are padding (is_valid = 0 over garbage): every other row is one access to one of
    n_locations random locations in address spaces 1 and 2, in random row order, with distinct timestamps; the chains per location
    are built by sorting. -> (cols u32[13, rows] canonical, the reference boundary trace)"""
    rng = np.random.default_rng([seed, log_rows])
    rows = 1 << log_rows
    n = rows - invalid
    keys = np.unique(rng.integers(0, 1 << 29, size=2 * n_locations) * 4 + rng.integers(1, 3, size=2 * n_locations))[:n_locations]
    rng.shuffle(keys)
    loc_as, loc_ptr = keys & 3, (keys >> 2) & ~np.int64(3)
    key2 = np.unique(loc_as << 32 | loc_ptr, return_index=True)[1]  # (distinct (as, ptr) after the alignment)
    loc_as, loc_ptr = loc_as[key2], loc_ptr[key2]
    L = len(loc_as)
    loc = np.concatenate([np.arange(min(L, n)), rng.integers(0, L, size=max(0, n - L))])[:n]  # every location at least once when n >= L
    rng.shuffle(loc)
    ts = 1000 + rng.permutation(n)
    new = rng.integers(0, 256, size=(4, n))
    order = np.lexsort((ts, loc))
    first = np.concatenate([[True], loc[order][1:] != loc[order][:-1]])
    last = np.concatenate([first[1:], [True]])
    prev = np.zeros((4, n), np.int64)
    prev_ts = np.zeros(n, np.int64)
    prev[:, order[1:]] = new[:, order[:-1]]
    prev_ts[order[1:]] = ts[order[:-1]]
    n_first = int(first.sum())
    init_bytes, init_ts = rng.integers(0, 256, size=(4, n_first)), rng.integers(0, 1000, size=n_first)
    prev[:, order[first]] = init_bytes
    prev_ts[order[first]] = init_ts
    cols = rng.integers(0, P, size=(13, rows))
    cols[0, :n], cols[1, :n] = loc_as[loc], loc_ptr[loc]
    cols[2:6, :n], cols[6, :n], cols[7:11, :n], cols[11, :n], cols[12, :n] = prev, prev_ts, new, ts, 1
    cols[12, n:] = 0
    touched = loc[order[first]]
    want = boundary_from_arrays(loc_as[touched], loc_ptr[touched], init_bytes, init_ts, new[:, order[last]], ts[order[last]])
    return cols.astype(np.uint32), want
