"""Segment proofs whose levels mix RESIDENT and STREAMED AIRs (segment_prover.hip), chosen AIR by AIR with the test hook
POWDR_STREAM_LOG_BLOCKS_BY_AIR instead of by chance through the memory policy.

A level of a mixed tree that holds a streamed matrix is absorbed run by run (commit_mixed, merkle.hip leaf_absorb_kernel): resident
runs through the column-pointer table, streamed runs sub-coset by sub-coset with their own sub-coset counts, the rows' sponge states
parked between the runs and the rate position carried over the run boundaries (widths that are no multiples of 8). The quotient,
DEEP and query phases then read resident and streamed AIRs side by side, handed-over (eaten) traces next to copied coefficients.
Every case: words == the oracle's (sm.prove_segment), both verifiers accept, segment_last_modes() == the forced modes and the eaten
flags, eaten traces restored bit-exactly, a second proof gives the same words (tests/test_segment_proof.hip_segment_consuming)."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from powdr_amd import synth
from tests.test_segment_proof import descs_of, gpu, hip_segment_consuming, to_dev  # noqa: F401  (gpu: the module fixture)

P = om.P
PA, PC, ADD, SUB, MUL = 0, 1, 2, 3, 4


def valid_air(w, lh, n_int, seed, n_cons=4):
    """A random 2^lh-row trace of w columns and constraint programs it satisfies (the forms of an optimised APC: a*b - t, t*(t - 1),
    a*b*c - t, a + k*b - t, each over its own target column t, the free columns random), n_int bus interactions over its columns
    (synth.random_air_programs). -> oracle air tuple (trace column-major, W, log_h, cons_bc, cons_spans, interactions)."""
    rng = np.random.default_rng(seed)
    H = 1 << lh
    t = rng.integers(0, P, size=(w, H), dtype=np.uint64)
    n_cons = min(n_cons, w - 1) if w > 1 else 1
    free = w - n_cons if w > 1 else 0
    src = lambda: int(rng.integers(0, free)) if free else 0
    bc, spans = [], []
    for k in range(n_cons):
        off, tc, form = len(bc), w - 1 - k, k % 4
        if w == 1 or form == 1:
            t[tc] = rng.integers(0, 2, H)
            bc += [PA, tc, PA, tc, PC, 1, SUB, MUL]
        elif form == 0:
            a, b = src(), src()
            t[tc] = t[a] * t[b] % P
            bc += [PA, a, PA, b, MUL, PA, tc, SUB]
        elif form == 2:
            a, b, c = src(), src(), src()
            t[tc] = t[a] * t[b] % P * t[c] % P
            bc += [PA, a, PA, b, MUL, PA, c, MUL, PA, tc, SUB]
        else:
            a, b, kk = src(), src(), int(rng.integers(1, 1 << 16))
            t[tc] = (t[a] + kk * t[b]) % P
            bc += [PA, a, PC, kk, PA, b, MUL, ADD, PA, tc, SUB]
        spans.append((off, len(bc) - off))
    it = synth.random_air_programs(w, 0, n_int, seed=seed)[2]
    return (np.ascontiguousarray(t.astype(np.uint32)).reshape(-1), w, lh, np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2), it)


# (width, log_h, interactions, forced log2(sub-cosets), handed over, word offset of the trace); AIRs of 2^3 .. 2^12 rows except g
CASES = {
    # a: one level R | S | R — three runs, the rate position carried over both boundaries (13 -> 5, + 7 -> 4); a taller resident AIR
    "a_resident_streamed_resident": [(13, 8, 3, 0, True, 0), (7, 8, 2, 2, True, 0), (11, 8, 4, 0, False, 0), (5, 10, 2, 0, True, 0)],
    # b: one level S(b=1) | R | S(b=3): runs with different sub-coset counts; a streamed AIR at the tallest level as well
    "b_two_subcoset_counts": [(9, 9, 3, 1, True, 0), (6, 9, 2, 0, True, 0), (19, 9, 4, 3, False, 0), (3, 11, 1, 2, True, 0)],
    # c: a streamed AIR alone at the tallest level; below it (injected digests) a streamed and a resident AIR share a level
    "c_streamed_top_mixed_below": [(10, 12, 3, 2, True, 0), (5, 6, 2, 2, True, 0), (12, 6, 3, 0, True, 0), (3, 4, 1, 0, False, 0)],
    # d: two streamed AIRs at one level, one eaten (coefficients in the caller's buffer), one copied (tcoef); a resident third
    "d_eaten_beside_copied": [(11, 7, 3, 2, True, 0), (5, 7, 2, 3, False, 0), (9, 7, 2, 0, True, 0), (6, 9, 2, 1, True, 0)],
    # e: LogUp with AIRs WITHOUT interactions in the mixed level (a streamed one and a resident one)
    "e_no_interactions_in_the_level": [(7, 8, 3, 1, True, 0), (6, 8, 0, 0, True, 0), (10, 8, 0, 2, False, 0), (4, 5, 0, 0, True, 0)],
    # f: a streamed AIR of width 1 (and its clamp: 5 asked, b_max = log_h - 1 = 3) beside a resident one of width 3
    "f_width_one": [(1, 4, 1, 5, True, 0), (3, 4, 2, 0, True, 0), (1, 7, 1, 2, False, 0), (6, 7, 2, 0, True, 0)],
    # g: 2^16 rows — a resident AIR whose trace sits at an ODD word offset (no DEEP combination path), a streamed AIR of the same
    # height and a resident aligned one (the combination path); a short AIR that may not stream (log_h < 3) asked to
    "g_tall_misaligned_resident": [(3, 16, 2, 0, False, 1), (5, 16, 2, 2, True, 0), (4, 16, 1, 0, False, 0), (2, 2, 1, 3, True, 0)],
}
PARAMS = {"a_resident_streamed_resident": (6, 2), "b_two_subcoset_counts": (5, 0), "c_streamed_top_mixed_below": (6, 3),
          "d_eaten_beside_copied": (4, 0), "e_no_interactions_in_the_level": (5, 2), "f_width_one": (6, 0), "g_tall_misaligned_resident": (3, 1)}
_AIRS, _WANT = {}, {}


def case_airs(name):
    if name not in _AIRS:
        _AIRS[name] = [valid_air(w, lh, n_int, seed=1000 * k + 17 * w + lh) for k, (w, lh, n_int, _, _, _) in enumerate(CASES[name])]
    return _AIRS[name]


def case_oracle(name, logup):
    if (name, logup) not in _WANT:
        nq, pb = PARAMS[name]
        _WANT[(name, logup)] = sm.prove_segment(case_airs(name), num_queries=nq, pow_bits=pb, logup=logup)
    return _WANT[(name, logup)]


def forced_modes(spec):
    """(log2 sub-cosets, eaten) the hook must produce: clamped to b_max = min(log_h - 1, 5), none below 2^3 rows."""
    out = []
    for w, lh, _, b, handed, _ in spec:
        bb = min(b, lh - 1, 5) if lh >= 3 else 0
        out.append((bb, bool(handed) and bb > 0))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("logup", [False, True])
def test_the_oracle_accepts_the_case(name, logup):
    """(CPU) the fixtures are valid: the oracle's proof of every case is accepted by the oracle verifier and the host verifier."""
    from powdr_amd import prover

    airs, nq, pb = case_airs(name), *PARAMS[name]
    want = case_oracle(name, logup)
    assert sm.verify_segment(want, airs, nq, pb, logup)[0] == 0
    assert prover.verify_segment(descs_of(airs), want, nq, pb, logup)[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("logup", [False, True])
@pytest.mark.parametrize("jit", ["0", "1"])
def test_mixed_levels_equal_the_oracle(gpu, monkeypatch, name, logup, jit):
    torch, abi, prover = gpu
    spec = CASES[name]
    airs, (nq, pb) = case_airs(name), PARAMS[name]
    want = case_oracle(name, logup)
    monkeypatch.delenv("POWDR_STREAM_LOG_BLOCKS", raising=False)
    monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS_BY_AIR", ",".join(str(s[3]) for s in spec))
    monkeypatch.setenv("POWDR_JIT", jit)
    got, modes = hip_segment_consuming(gpu, airs, nq, pb, logup, [s[4] for s in spec], offsets=[s[5] for s in spec])
    assert modes == forced_modes(spec)
    assert prover.segment_last_plan() == (0, 0, 0)  # forced: no policy ran
    assert len(got) == len(want) and (got == want).all(), f"first differing word {int(np.argmax(got != want))} of {len(want)}"
    assert prover.verify_segment(descs_of(airs), got, nq, pb, logup)[0] == 0
    assert sm.verify_segment(got, airs, nq, pb, logup)[0] == 0


@pytest.mark.gpu
def test_the_per_air_hook_refuses_a_list_of_another_length(gpu, monkeypatch):
    """A POWDR_STREAM_LOG_BLOCKS_BY_AIR list whose length is not the number of AIRs (or that is no list of counts) fails the call
    with hipErrorInvalidValue before any trace is touched, handed over or not. pw_segment_last_modes counts without a buffer."""
    torch, abi, prover = gpu
    name = "d_eaten_beside_copied"
    airs, (nq, pb) = case_airs(name), PARAMS[name]
    provers = [prover.Prover(a[1], a[3], a[4], num_queries=nq, pow_bits=pb) for a in airs]
    orig = [to_dev(torch, a[0]) for a in airs]
    traces = [t.clone() for t in orig]
    seg = [(pr, t.data_ptr(), a[2]) for pr, t, a in zip(provers, traces, airs)]
    monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS_BY_AIR", "2,2,2,2")
    want = prover.prove_segment(seg, hand_over=[False] * 4)
    assert int(prover.lib.pw_segment_last_modes(None, 8)) == 4  # NULL out with a capacity: the count only
    for bad in ("2,2,2", "2,2,2,2,2", "2,x,2,2", "2,,2,2", "2,-1,2,2", ""):
        monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS_BY_AIR", bad)
        with pytest.raises(Exception):
            prover.prove_segment(seg, hand_over=True)
        torch.cuda.synchronize()
        assert all(torch.equal(t, o) for t, o in zip(traces, orig)), bad
    monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS_BY_AIR", "2,2,2,2")
    assert (prover.prove_segment(seg, hand_over=[False] * 4) == want).all()
    for pr in provers:
        pr.close()
