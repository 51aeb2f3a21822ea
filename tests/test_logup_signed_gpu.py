"""The LogUp permutation and quotient kernels on the signed extension arithmetic (csrc/ext.hpp bb::SExt, csrc/jit_device.hpp), through
the stage entry points of tests/test_stage_logup_gpu.py, word for word against tests/_stage_ref.py AND against the other path of the
same prover (POWDR_JIT=0: the interpreter twins; POWDR_JIT=1: the specialised kernels, in one chunk and in two).

The AIR is built around the places where the signed code takes another branch:
  * interactions with 0, 1, 4, 5, 8 and 9 arguments: pwj::DenominatorAcc folds after every fourth term (bb::bounds::kDenTermsPerFold),
    so these sit on both sides of the first and the second fold;
  * groups of 1, 2, 3 and 5 members: q d0 - m0, the closed two-member form, one and three turns of num <- num d + den m. (A group has at
    least one member — logup_group_starts never makes an empty one — so the generated code's n = 0 line cannot be reached from here.)
  * AIRs of 1, 4, 5 and 9 groups (the first groups of the same table): every remainder of the batches of four that share an inversion;
    with POWDR_JIT_CHUNK_COST = 2600 the nine groups fall into two chunks of 4 and 5;
  * heights 2^1 and 2^9 (two workgroups); every fourth row has all multiplicities zero, next to rows that do not;
  * cells and multiplicities from tests/_edge_values.EDGE: 0, 1, p - 1, (p - 1) / 2, (p + 1) / 2 as values and as device words;
  * challenge tables (alpha, blpow, apow) whose centred coordinates are (p - 1) / 2, -(p - 1) / 2 and 0 — what no transcript makes;
  * a denominator that vanishes (test_stage_logup_gpu.vanishing_inputs)."""
import numpy as np
import pytest

from oracle import apc_model as om
from tests import _edge_values as ev
from tests import _stage_ref as ref
from tests._edge_values import MUL, PA, PC, SUB, _programs
from tests.test_prover_gpu import gpu  # noqa: F401  (the module-level fixture: torch, abi, prover — or a skip without a GPU)
from tests.test_stage_kernels_gpu import ALL_PM1, ZERO4, rand_ext
from tests.test_stage_logup_gpu import (_ENV, WORD_HI, WORD_LO, cells, first_difference, group_starts, multiplicity_columns, perm_columns, run_perm,
                                        run_quotient, vanishing_inputs)

P = om.P
KINDS = {
    "interpreter": {"POWDR_JIT": "0"},
    "jit": {"POWDR_JIT": "1", "POWDR_JIT_MIN_LOG_HEIGHT": "1"},
    "jit-two-chunks": {"POWDR_JIT": "1", "POWDR_JIT_MIN_LOG_HEIGHT": "1", "POWDR_JIT_CHUNK_COST": "2600"},
}
# (column arguments, constant arguments, the first argument a product of two columns) per interaction; the groups they fall into
TABLE = [
    [(1, 0, True)],                                                        # a group of one: its argument has degree 2
    [(4, 0, False), (5, 0, False)],
    [(8, 0, False), (9, 0, False), (0, 0, False)],
    [(1, 0, False), (0, 4, False), (0, 9, False), (5, 0, False), (0, 0, False)],
    [(8, 0, False), (1, 0, False)],
    [(4, 0, True)],
    [(9, 0, False), (5, 0, False)],
    [(4, 0, False), (0, 0, False), (8, 0, False)],
    [(1, 0, False), (0, 5, False)],
]
GROUP_COUNTS = [1, 4, 5, 9]
FAMILIES = ["random", "edge", "centred"]
LOG_HEIGHTS = (1, 9)


def fold_air(n_groups):
    """the first n_groups groups of TABLE: two constraints, every multiplicity and column argument a column of its own"""
    col = lambda c: [PA, c]
    nxt, interactions = 3, []
    for g, members in enumerate(TABLE[:n_groups]):
        for k, (n_col, n_const, product) in enumerate(members):
            mult, args = col(nxt), []
            nxt += 1
            for j in range(n_col):
                args.append(col(nxt) + col(nxt + 1) + [MUL] if product and j == 0 else col(nxt))
                nxt += 2 if product and j == 0 else 1
            args += [[PC, int(ev.EDGE[(g + k + j) % len(ev.EDGE)])] for j in range(n_const)]
            interactions.append((2 + g % 3, mult, args))
    cons, it = _programs([col(0) + col(1) + [MUL] + col(2) + [SUB], col(1) + col(2) + [MUL] + col(0) + [SUB]], interactions)
    assert np.diff(group_starts(it)).tolist() == [len(m) for m in TABLE[:n_groups]]
    return nxt, cons, it


def centred_table(rng, n):
    """(n, 4) canonical coordinates whose device words are centred at (p - 1) / 2, -(p - 1) / 2 or 0"""
    return np.array([WORD_HI, WORD_LO, 0], np.uint32)[rng.integers(0, 3, (n, 4))]


def tables(family, rng, n):
    return centred_table(rng, n) if family == "centred" else cells(family, rng, n, 4)


@pytest.fixture(scope="module")
def provers(gpu):
    """get(n_groups, kind) -> (Prover, W, cons, it), made once per module"""
    torch, abi, prover = gpu
    made = {}

    def get(n_groups, kind):
        if (n_groups, kind) not in made:
            W, cons, it = fold_air(n_groups)
            with pytest.MonkeyPatch.context() as mp:
                for k in _ENV:
                    mp.delenv(k, raising=False)
                for k, v in KINDS[kind].items():
                    mp.setenv(k, v)
                pr = prover.Prover(W, cons[0], cons[1], num_queries=4, pow_bits=0, interactions=it)
                if kind != "interpreter":
                    assert pr.specialise(), pr.specialised()
            info = pr.specialised()
            if kind == "interpreter":
                assert info["state"] != 1
            if kind == "jit-two-chunks":  # the constraints' chunk, and two chunks of groups in either kernel
                assert info["chunks"] == 5, info
            made[(n_groups, kind)] = (pr, W, cons, it)
        return made[(n_groups, kind)]

    yield get
    torch.cuda.synchronize()
    for pr, *_ in made.values():
        pr.close()


def kinds_of(n_groups):
    return list(KINDS) if n_groups == 9 else ["interpreter", "jit"]


def perm_case(rng, family, W, it, log_h):
    H = 1 << log_h
    T = cells("random" if family == "centred" else family, rng, W, H)
    T[sorted({c for cs in multiplicity_columns(it) for c in cs}), 1::4] = 0  # no inversion on these rows, next to rows with one
    n_bl = int(it[0][:, 1].max()) + 2
    return T, tuple(int(x) for x in tables(family, rng, 1)[0]), tables(family, rng, n_bl)


@pytest.mark.gpu
@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_permutation_columns(gpu, provers, n_groups):
    """pwj_perm_* and logup_perm_kernel: the group columns, the row sums and phi, equal to the reference and to each other"""
    _, W, cons, it = provers(n_groups, "interpreter")
    starts = group_starts(it)
    for log_h in LOG_HEIGHTS:
        for f, family in enumerate(FAMILIES):
            T, alpha, blpow = perm_case(np.random.default_rng([11, n_groups, log_h, f]), family, W, it, log_h)
            q, rowsum, phi = ref.logup_perm(T, it, starts, alpha, blpow)
            seen = {}
            for kind in kinds_of(n_groups):
                got, got_rs, clean = run_perm(gpu, provers(n_groups, kind)[0], it, T, log_h, alpha, blpow)
                want = perm_columns(q, phi, rowsum if kind != "interpreter" else None)
                assert clean, (kind, log_h, family)
                assert (got == want).all(), (kind, log_h, family, "column, row", first_difference(got, want))
                assert (got_rs == rowsum).all(), (kind, log_h, family, "row, coordinate", first_difference(got_rs, rowsum))
                seen[kind] = got[:4 * n_groups + 4]
            for kind in seen:
                assert (seen[kind] == seen["interpreter"]).all(), (kind, log_h, family)


@pytest.mark.gpu
def test_vanishing_denominator(gpu, provers):
    """the second member of the three-member group has the denominator 0 on four rows: that group's ONE inversion is of 0 and leaves
    q = 0 there, its batch partners keep their inverses; every path alike"""
    _, W, cons, it = provers(9, "interpreter")
    starts = group_starts(it)
    for log_h in LOG_HEIGHTS:
        T, alpha, blpow, i, rows = vanishing_inputs("fold", np.random.default_rng([12, log_h]), W, it, log_h)
        q, rowsum, phi = ref.logup_perm(T, it, starts, alpha, blpow, vanishing=[(i, r) for r in rows])
        g = [k for k in range(len(starts) - 1) if starts[k] <= i < starts[k + 1]][0]
        assert starts[g + 1] - starts[g] == 3 and not q[g][rows].any()
        for kind in KINDS:
            got, got_rs, clean = run_perm(gpu, provers(9, kind)[0], it, T, log_h, alpha, blpow)
            want = perm_columns(q, phi, rowsum if kind != "interpreter" else None)
            assert clean and (got == want).all() and (got_rs == rowsum).all(), (kind, log_h, first_difference(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_quotient(gpu, provers, n_groups):
    """pwj_quotient_* + the tail, quotient_logup_kernel: q den - num under centred-extreme alpha powers, permutation cells at the edges"""
    _, W, cons, it = provers(n_groups, "interpreter")
    starts = group_starts(it)
    G, nc = n_groups, len(cons[1])
    for log_n in LOG_HEIGHTS:
        N = 1 << log_n
        for f, family in enumerate(FAMILIES):
            rng = np.random.default_rng([13, n_groups, log_n, f])
            lde = cells("random" if family == "centred" else family, rng, W, N)
            plde = np.zeros((4 * G + 8, N), np.uint32)
            plde[:4 * G + 4] = cells("random" if family == "random" else "edge", rng, 4 * G + 4, N)
            plde[4 * G + 4:] = plde[:4 * G].reshape(G, 4, N).astype(np.uint64).sum(axis=0) % P
            apow, blpow = tables(family, rng, nc + G + 3), tables(family, rng, int(it[0][:, 1].max()) + 2)
            alpha = tuple(int(x) for x in tables(family, rng, 1)[0])
            for S in (ZERO4, ALL_PM1, rand_ext(rng)):
                want = ref.quotient(lde, plde, log_n, cons, it, starts, apow, alpha, blpow, S).T
                for kind in kinds_of(n_groups):
                    got, clean, _ = run_quotient(gpu, provers(n_groups, kind)[0], it, lde, plde, log_n, apow, alpha, blpow, S)
                    assert clean and (got == want).all(), (kind, log_n, family, S, "coordinate, row", first_difference(got, want))
