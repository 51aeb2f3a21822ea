"""The bus half of the mock prover, pw_check_segment_buses — what can be checked without a GPU: the symbol and its
three statements (header, Rust ffi, ctypes), the argument checks (refused before any GPU call), and the numpy reference the GPU tests
compare against (tests/_bus_multiset.py) on an example small enough to tally by hand."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from tests import _bus_multiset as bm

ROOT = Path(__file__).resolve().parents[1]
P = bm.P


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "powdr_prover.h").read_text(), flags=re.S)


def test_symbol_header_ffi_and_ctypes_agree():
    from powdr_amd import prover

    for name in ("pw_check_segment_buses", "pw_bus_check_scratch_bytes", "pw_bus_check_peak_bytes", "pw_bus_check_last_stats"):
        assert hasattr(prover.lib, name), name
        assert name in prover.PROVER_SYMBOLS
    hdr, ffi = _header(), (ROOT / "rust" / "powdr-hip" / "src" / "ffi.rs").read_text()
    m = re.search(r"\bpw_check_segment_buses\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    c_params = [re.findall(r"(\w+)\s*$", x.strip())[0] for x in m.group(1).split(",")]
    r = re.search(r"pub fn pw_check_segment_buses\s*\(([^;]*?)\)\s*->", ffi, flags=re.S)
    assert re.findall(r"(\w+)\s*:", r.group(1)) == c_params
    assert len(prover.lib.pw_check_segment_buses.argtypes) == len(c_params) == 13
    for name, cls in (("PwBusSummary", prover.PwBusSummary), ("PwBusTuple", prover.PwBusTuple)):
        body = re.search(r"typedef struct\s+" + name + r"\s*\{([^}]*)\}\s*" + name + r"\s*;", hdr, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            if decl.strip():
                c_fields += [re.sub(r"\[.*?\]", "", x).split()[-1].strip("* ") for x in decl.split(",")]
        rust = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct " + name + r"\s*\{([^}]*)\}", ffi, flags=re.S).group(1)
        assert re.findall(r"pub (\w+)\s*:", rust) == c_fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(prover.PwBusSummary) == 24 and C.sizeof(prover.PwBusTuple) == 104
    assert re.search(r"#define PW_BUS_MAX_ARGS 16u", hdr) and re.search(r"pub const PW_BUS_MAX_ARGS: usize = 16;", ffi) and prover.PW_BUS_MAX_ARGS == 16
    assert re.search(r"#define PW_BUS_CHECK_TALLY_ALL 1u", hdr) and re.search(r"pub const PW_BUS_CHECK_TALLY_ALL: u32 = 1;", ffi)


def test_malformed_arguments_are_refused_without_a_gpu():
    from powdr_amd import prover

    f = prover.lib.pw_check_segment_buses
    sums, tups = (prover.PwBusSummary * 4)(), (prover.PwBusTuple * 4)()
    ns, nt = C.c_size_t(), C.c_size_t()
    one = (prover.PwSegmentAir * 1)()
    # NULL airs with n > 0
    assert f(None, 1, None, 0, 0, 0, 0, sums, 4, C.byref(ns), tups, 4, C.byref(nt)) == -1
    # summaries wanted with room for none
    assert f(one, 0, None, 0, 0, 0, 0, sums, 0, C.byref(ns), tups, 4, C.byref(nt)) == -1
    # a NULL prover (and a NULL trace)
    one[0] = prover.PwSegmentAir(None, 16, 3, 0)
    assert f(one, 1, None, 0, 0, 0, 0, sums, 4, C.byref(ns), tups, 4, C.byref(nt)) == -1
    # a bus list that is not there, an unknown flag, tuples without a count
    assert f(one, 0, None, 2, 0, 0, 0, sums, 4, C.byref(ns), tups, 4, C.byref(nt)) == -1
    assert f(one, 0, None, 0, 0, 0, 2, sums, 4, C.byref(ns), tups, 4, C.byref(nt)) == -1
    assert f(one, 0, None, 0, 0, 0, 0, sums, 4, C.byref(ns), tups, 4, None) == -1
    # more buses than summaries
    ids = np.arange(5, dtype=np.uint32)
    assert f(one, 0, ids.ctypes.data_as(C.c_void_p), 5, 0, 0, 0, sums, 4, C.byref(ns), tups, 4, C.byref(nt)) == -1
    # nothing to check is not an error (and still touches no GPU)
    assert f(one, 0, None, 0, 0, 0, 0, sums, 4, C.byref(ns), tups, 4, C.byref(nt)) == 0 and ns.value == 0 and nt.value == 0


# post-fix code: 0 PUSH column, 1 PUSH constant, 3 SUB
COL = lambda c: [0, c]
NEG_COL = lambda c: [1, 0, 0, c, 3]


def _program(interactions):
    """[(bus, [mult code, arg code, ...])] -> (inter, spans, bytecode)"""
    inter, spans, bc = [], [], []
    for bus, codes in interactions:
        inter.append([bus, len(codes) - 1, len(spans)])
        for code in codes:
            spans.append([len(bc), len(code)])
            bc += code
    return np.array(inter, np.uint32), np.array(spans, np.uint32), np.array(bc, np.uint32)


def hand_example():
    """Ten rows in two AIRs. AIR 0 (6 rows; columns m, a, b, h) sends (a, b) on bus 5 with multiplicity m and (h) on bus 9 with
    multiplicity h2 = column 4; AIR 1 (4 rows; columns m, a, b) receives (a, b, 0) on bus 5 — THREE arguments — and (a, b) on bus 5
    through a second interaction."""
    half = (P + 1) // 2
    air0 = np.array([
        # m  a  b  h   h2
        [1, 7, 8, 3, half],       # (7, 8) +1 ; bus 9: (3) + (p + 1) / 2
        [2, 7, 8, 3, half - 1],   # (7, 8) +2 ; bus 9: (3) + (p - 1) / 2   -> bus 9 sums to exactly p: balanced
        [0, 9, 9, 4, 0],          # inactive on both
        [1, 1, 2, 5, 1],          # (1, 2) +1 ; bus 9: (5) + 1
        [P - 1, 1, 2, 5, P - 1],  # (1, 2) -1 -> cancels inside the AIR ; bus 9: (5) - 1 -> cancels
        [1, 4, 4, 6, 0],          # (4, 4) +1, received below as (4, 4)
    ], dtype=np.int64).T
    air1 = np.array([
        # m  a  b   m2
        [3, 7, 8, 0],             # receives (7, 8, 0) three times: NOT the tuple (7, 8)
        [0, 0, 0, 1],             # receives (0, 0) once through the second interaction: never sent
        [0, 4, 4, 1],             # receives (4, 4): balances row 5 of AIR 0
        [0, 0, 0, 0],
    ], dtype=np.int64).T
    it0 = _program([(5, [COL(0), COL(1), COL(2)]), (9, [COL(4), COL(3)])])
    it1 = _program([(5, [NEG_COL(0), COL(1), COL(2), [1, 0]]), (5, [NEG_COL(3), COL(1), COL(2)])])
    return [(air0, it0), (air1, it1)]


def test_numpy_reference_on_a_hand_written_example():
    airs = hand_example()
    table, active = bm.tally(airs)
    assert active == {5: 5 + 1 + 2, 9: 4}
    assert table[(9, 1, (3,))] == [0, (0, 1, 0), 2]                # (p + 1) / 2 + (p - 1) / 2 = p = 0
    assert table[(9, 1, (5,))] == [0, (0, 1, 3), 2]
    assert table[(5, 2, (1, 2))] == [0, (0, 0, 3), 2]
    assert table[(5, 2, (4, 4))] == [0, (0, 0, 5), 2]
    assert table[(5, 2, (7, 8))] == [3, (0, 0, 0), 2]              # sent 1 + 2, received by nobody as a PAIR
    assert table[(5, 3, (7, 8, 0))] == [P - 3, (1, 0, 0), 1]       # the triple is another tuple
    assert table[(5, 2, (0, 0))] == [P - 1, (1, 1, 1), 1]
    summaries, tuples = bm.expected(airs)
    assert summaries == [dict(bus=5, status=1, n_active=8, n_unbalanced=3), dict(bus=9, status=0, n_active=4, n_unbalanced=0)]
    # ordered by (bus, n_args, args): the pairs before the triple, (0, 0) before (7, 8)
    assert [(t["n_args"], t["args"], t["net_multiplicity"]) for t in tuples] == [(2, [0, 0], P - 1), (2, [7, 8], 3), (3, [7, 8, 0], P - 3)]
    assert [(t["air"], t["interaction"], t["row"], t["n_contributions"]) for t in tuples] == [(1, 1, 1, 1), (0, 0, 0, 2), (1, 0, 0, 1)]
    # in the LogUp sum (a, b) and (a, b, 0) coincide: there, (7, 8) and (7, 8, 0) would cancel — here they must not
    only9 = bm.expected(airs, buses=[9])
    assert only9 == ([dict(bus=9, status=0, n_active=4, n_unbalanced=0)], [])
    assert bm.expected(airs, buses=[77])[0] == [dict(bus=77, status=0, n_active=0, n_unbalanced=0)]
