"""The run-time specialised kernels' generated code EXECUTED ON THE HOST, and what it must compute (shared by test_jit.py and
test_edge_values_cpu.py). The generated translation units are plain C++ over the embedded headers, so a shim (`__global__` = nothing,
blockIdx / threadIdx = globals) builds them with the host compiler; the expected values are plain Python integers in F_p[X]/(X^4 - 11).
This is the only place where the challenges (alpha, the powers of beta, the powers of the constraint challenge) are the caller's."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

from oracle import apc_model as om

P = om.P
PA, PC, ADD, SUB, MUL, NEG = om.OP_PUSH_APC, om.OP_PUSH_CONST, om.OP_ADD, om.OP_SUB, om.OP_MUL, om.OP_NEG

_SHIM = """
#include <cstddef>
#include <cstdint>
#include <cstring>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
static struct { unsigned x, y, z; } blockIdx, threadIdx;
"""
_W4 = 11  # F_p[X] / (X^4 - 11)


def _ext_mul(a, b):
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return [(c[k] + _W4 * (c[k + 4] if k < 3 else 0)) % P for k in range(4)]


def _ext_add(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def _ext_scale(a, s):
    return [x * s % P for x in a]


def _ext_inv(a):
    r, base, e = [1, 0, 0, 0], list(a), P ** 4 - 2
    while e:
        if e & 1:
            r = _ext_mul(r, base)
        base = _ext_mul(base, base)
        e >>= 1
    return r


def ext_inv_tower(a):
    """the same inverse through the tower F_p[Y]/(Y^2 - 11), Y = X^2 (one base-field power instead of a 124-bit one); the product with
    `a` is checked on the spot, so a slip here cannot pass for a value"""
    a0, a1, a2, a3 = (int(x) for x in a)
    # a = A + X B, A = a0 + a2 Y, B = a1 + a3 Y;  1/a = (A - X B) / (A^2 - Y B^2)
    d0 = (a0 * a0 + _W4 * a2 * a2 - 2 * _W4 * a1 * a3) % P
    d1 = (2 * a0 * a2 - a1 * a1 - _W4 * a3 * a3) % P
    n = pow((d0 * d0 - _W4 * d1 * d1) % P, P - 2, P)
    e0, e1 = d0 * n % P, -d1 * n % P  # 1 / (d0 + d1 Y)
    inv = [(a0 * e0 + _W4 * a2 * e1) % P, -(a1 * e0 + _W4 * a3 * e1) % P, (a0 * e1 + a2 * e0) % P, -(a1 * e1 + a3 * e0) % P]
    assert _ext_mul(inv, [a0, a1, a2, a3]) == [1, 0, 0, 0], "a LogUp denominator that vanishes: choose other challenges"
    return inv


def eval_postfix(code, row):
    """a post-fix program on one row's cells (-> a Python integer), or on every row at once when `row` is the whole W x n matrix
    (-> n int64 words: a product of two words stays below 2^62, and % of a negative int64 is non-negative). Cells that are no integers
    (elements of a ring with + - * and % of its own: openings in the extension field) are taken as they are."""
    whole = getattr(row, "ndim", 1) == 2
    st, i = [], 0
    while i < len(code):
        op = int(code[i])
        if op in (PA, PC):
            cell = row[int(code[i + 1])] if op == PA else int(code[i + 1]) % P
            st.append(cell.astype(np.int64) if whole and op == PA else int(cell) if isinstance(cell, (int, np.integer)) else cell)
            i += 2
        elif op == NEG:
            st.append(-st.pop() % P)
            i += 1
        else:
            y, x = st.pop(), st.pop()
            st.append((x + y) % P if op == ADD else (x - y) % P if op == SUB else x * y % P)
            i += 1
    return st[0]


def expected_values(bc, spans, it, starts, canon, N, ext_inv=_ext_inv):
    """(q_want[n_groups, N, 4], quot_want[N, 4]), canonical, for canon = {"T", "Pm", "apow", "al", "blpow"}:
      * the LogUp permutation columns q_g = sum_{i in g} m_i / (alpha + bus_i + sum_j beta^(j+1) a_ij),
      * the quotient numerator sum_c alpha^c C_c + sum_g alpha^(nc+g) (q_g prod d_i - sum_i m_i prod_{l != i} d_l) with the committed
        (here: the caller's) q_g of `Pm`."""
    inter, ispans, ibc = it
    n_groups, n_cons = len(starts) - 1, len(spans)
    T = canon["T"]
    al, bl = [int(x) for x in canon["al"]], [[int(x) for x in b] for b in canon["blpow"]]
    q_want = np.zeros((n_groups, N, 4), np.int64)
    quot_want = np.zeros((N, 4), np.int64)
    for r in range(N):
        row = T[:, r]
        acc = [0, 0, 0, 0]
        for c, (off, ln) in enumerate(spans.tolist()):
            acc = _ext_add(acc, _ext_scale([int(x) for x in canon["apow"][c]], eval_postfix(bc[off:off + ln], row)))
        for g in range(n_groups):
            ms, ds = [], []
            for i in range(int(starts[g]), int(starts[g + 1])):
                bus, n_args, s0 = (int(x) for x in inter[i])
                ev = lambda s: eval_postfix(ibc[int(ispans[s][0]):int(ispans[s][0]) + int(ispans[s][1])], row)
                ms.append(ev(s0))
                d = _ext_add(al, [bus % P, 0, 0, 0])
                for j in range(n_args):
                    d = _ext_add(d, _ext_scale(bl[j + 1], ev(s0 + 1 + j)))  # blpow[k] = beta^k: argument j meets beta^(j+1)
                ds.append(d)
            q = [0, 0, 0, 0]
            for m, d in zip(ms, ds):
                q = _ext_add(q, _ext_scale(ext_inv(d), m))
            q_want[g, r] = q
            pq = [int(canon["Pm"][4 * g + k, r]) for k in range(4)]  # the committed (here: the caller's) q_g the quotient reads
            prod_all = [1, 0, 0, 0]
            for d in ds:
                prod_all = _ext_mul(prod_all, d)
            term = _ext_mul(pq, prod_all)
            for i, m in enumerate(ms):
                rest = [1, 0, 0, 0]
                for l, d in enumerate(ds):
                    if l != i:
                        rest = _ext_mul(rest, d)
                term = _ext_add(term, _ext_scale(rest, -m % P))
            acc = _ext_add(acc, _ext_mul([int(x) for x in canon["apow"][n_cons + g]], term))
        quot_want[r] = acc
    return q_want, quot_want


def _build_units_for_the_host(tmp_path, units, which, total_chunks):
    """Every unit: shim + generated source + a driver that walks (chunk, row) like the grid would; built with the host compiler of the
    ROCm LLVM (plain C++: the embedded headers have host paths for everything), loaded with ctypes."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if Path("/opt/rocm/lib/llvm/bin/clang++").exists() else shutil.which("g++")
    csrc = Path(__file__).resolve().parents[1] / "powdr_amd" / "csrc"
    fns = []
    for k, u in enumerate(units):
        if which == 0:
            driver = f"""
extern "C" void run(const uint32_t* T, const uint32_t* Pm, size_t N, const bb::Ext* apow, const uint32_t* al4, const bb::Ext* blpow, uint32_t* part, uint32_t* unused) {{
    bb::Ext al; memcpy(&al, al4, 16);
    for (unsigned y = 0; y < {u['n_chunks']}u; ++y) for (size_t j = 0; j < N; ++j) {{
        blockIdx.x = (unsigned)(j / 256); blockIdx.y = y; threadIdx.x = (unsigned)(j % 256);
        {u['kernel']}(T, Pm, N, apow, al, blpow, part);
    }}
}}"""
        else:
            driver = f"""
extern "C" void run(const uint32_t* T, const uint32_t* Pm, size_t N, const bb::Ext* apow, const uint32_t* al4, const bb::Ext* blpow, uint32_t* perm, uint32_t* rowsum) {{
    bb::Ext al; memcpy(&al, al4, 16);
    for (unsigned y = 0; y < {u['n_chunks']}u; ++y) for (size_t j = 0; j < N; ++j) {{
        blockIdx.x = (unsigned)(j / 256); blockIdx.y = y; threadIdx.x = (unsigned)(j % 256);
        {u['kernel']}(T, N, al, blpow, perm, rowsum);
    }}
}}"""
        src = tmp_path / f"unit_{which}_{total_chunks}_{k}.cpp"
        src.write_text(_SHIM + u["source"] + driver)
        so = src.with_suffix(".so")
        subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-shared", "-fPIC", f"-I{csrc}", str(src), "-o", str(so)], check=True, capture_output=True)
        fn = C.CDLL(str(so)).run
        fn.restype = None
        fn.argtypes = [C.c_void_p] * 2 + [C.c_size_t] + [C.c_void_p] * 5
        fns.append(fn)
    return fns


def _call_units(fns, arrays, n_rows):
    for fn in fns:
        fn(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in (arrays["T"], arrays["Pm"], n_rows, arrays["apow"], arrays["al"], arrays["blpow"], arrays["out0"],
                                                                         arrays["out1"])])


class GeneratedCodeOnTheHost:
    """The generated code of one AIR for one chunking (`chunk_cost`, 2 chunks per unit), both kernel families (which = 1: the LogUp
    permutation columns, which = 0: the quotient numerator), compiled once; check() runs it on one set of inputs."""

    def __init__(self, tmp_path, W, bc, spans, it, chunk_cost):
        from powdr_amd import prover

        self.n_groups = len(prover.logup_group_starts(it)) - 1
        self.units, self.total, self.fns = {}, {}, {}
        for which in (1, 0):
            self.units[which], self.total[which] = prover.jit_generated_sources(W, bc, spans, it, which, chunk_cost, 2)
            self.fns[which] = _build_units_for_the_host(tmp_path, self.units[which], which, self.total[which])

    def check(self, canon, N, q_want, quot_want, what=""):
        """the perm columns, the row sums and the quotient parts equal the expected values"""
        monty = {k: om.to_monty(np.ascontiguousarray(v, np.uint32)) for k, v in canon.items()}
        n_groups = self.n_groups
        for which in (1, 0):
            total = self.total[which]
            out0 = np.zeros((max(total, n_groups) * 4 + 4, N), np.uint32) if which == 0 else np.zeros((4 * n_groups + 4, N), np.uint32)
            out1 = np.zeros((total * 4, N), np.uint32)
            _call_units(self.fns[which], dict(monty, out0=out0, out1=out1), N)
            if which == 1:
                got_q = om.from_monty(out0[:4 * n_groups]).astype(np.int64).reshape(n_groups, 4, N).transpose(0, 2, 1)
                assert (got_q == q_want).all(), what
                rowsum = om.from_monty(out1).astype(np.int64).reshape(total, 4, N).sum(axis=0) % P
                assert (rowsum.T == q_want.sum(axis=0) % P).all(), what
            else:
                parts = om.from_monty(out0[:total * 4]).astype(np.int64).reshape(total, 4, N).sum(axis=0) % P
                assert (parts.T == quot_want).all(), what
