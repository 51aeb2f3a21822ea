"""The memory policy of a segment proof (segment_prover.hip pw::plan_segment_streams) as a pure function of byte tables: which AIRs
are streamed over how many sub-cosets when the resident plan does not fit. CPU tests on hand-made tables, through the library's
test hook pw_segment_stream_plan, against a plain restatement of the rule (model_plan) and against the properties the rule promises:
round by round (TWO sub-cosets for the largest AIRs until the segment fits, four only when every AIR that may stream has two, ...),
largest first with ties in index order, each AIR's b_max respected, no step that does not shrink an AIR, and a plan that only grows
as the room shrinks. The GPU side (tests/test_segment_proof.py, tests/test_segment_mixed_modes_gpu.py) checks the real calls."""
import numpy as np
import pytest

from powdr_amd import prover


def model_plan(resident, streamed, b_max, own, avail):
    """The rule, restated: sizes sorted once (stable, largest first); rounds b = 1..5, in each the AIRs in that order take 2^b
    sub-cosets while the segment does not fit, skipping AIRs whose b_max is below b or whose streamed size is not smaller."""
    A = len(resident)
    cur, sbv = list(resident), [0] * A
    need = own + sum(cur)
    order = sorted(range(A), key=lambda a: -resident[a])
    for b in range(1, 6):
        for a in order:
            if need <= avail:
                return sbv, need
            if b > b_max[a] or streamed[a][b - 1] >= cur[a]:
                continue
            need += streamed[a][b - 1] - cur[a]
            cur[a], sbv[a] = streamed[a][b - 1], b
    return sbv, need


def planned_bytes(resident, streamed, own, sbv):
    return own + sum(r if b == 0 else s[b - 1] for r, s, b in zip(resident, streamed, sbv))


def shrinking_tables(rng, A, ties=False):
    """Streamed sizes that fall with every doubling of the sub-coset count and lie below the resident size (the usual case: the LDE
    goes, coefficients and a sub-coset buffer come)."""
    res = rng.integers(1, 4 if ties else 1 << 30, A).astype(np.int64) * (1 << 20 if ties else 1)
    fixed = (res * rng.uniform(0.2, 0.5, A)).astype(np.int64)
    streamed = [[int(fixed[a] + (res[a] - fixed[a]) // (2 << b)) for b in range(5)] for a in range(A)]
    b_max = [int(x) for x in rng.integers(0, 6, A)]
    return [int(x) for x in res], streamed, b_max


def check_round_order(resident, b_max, sbv, streamed=None):
    """No AIR that may stream sits at b - 2 while another sits at b; in the last round the AIRs raised form a prefix of the size
    order (stable, largest first) of the AIRs that may take that round. With `streamed` (real tables) only the AIRs that every
    further sub-coset doubling makes smaller are held to it: the others are passed by where a step would not shrink them."""
    B = max(sbv, default=0)
    held = [b_max[a] > 0 for a in range(len(sbv))]
    if streamed is not None:
        held = [h and all(x > y for x, y in zip([resident[a]] + list(streamed[a][:b_max[a]]), streamed[a][:b_max[a]])) for a, h in enumerate(held)]
    for a, b in enumerate(sbv):
        assert b <= b_max[a]
        if held[a]:
            assert b >= min(B - 1, b_max[a]), (a, sbv, b_max)
    if B:
        order = [a for a in sorted(range(len(sbv)), key=lambda a: -resident[a]) if held[a] and b_max[a] >= B]
        raised = [sbv[a] == B for a in order]
        assert raised == sorted(raised, reverse=True), (order, sbv)


def test_the_policy_equals_the_restated_rule_on_random_tables():
    rng = np.random.default_rng(5)
    for trial in range(400):
        A = int(rng.integers(1, 9))
        if trial % 3 == 0:  # arbitrary streamed sizes: some larger than resident, some not falling with b
            resident = [int(x) for x in rng.integers(1, 1000, A)]
            streamed = [[int(x) for x in rng.integers(1, 1200, 5)] for _ in range(A)]
            b_max = [int(x) for x in rng.integers(0, 6, A)]
        else:
            resident, streamed, b_max = shrinking_tables(rng, A, ties=trial % 3 == 1)
        own = int(rng.integers(0, 1 << 20))
        total = own + sum(resident)
        avail = int(rng.integers(0, total + 2))
        got, need = prover.segment_stream_plan(resident, streamed, b_max, own, avail)
        want, want_need = model_plan(resident, streamed, b_max, own, avail)
        assert (got, need) == (want, want_need), (resident, streamed, b_max, own, avail)
        assert need == planned_bytes(resident, streamed, own, got)
        if need > avail:
            # nothing more helps: no AIR has a larger sub-coset count left that would make it smaller
            for a in range(A):
                b = got[a]
                cur = resident[a] if b == 0 else streamed[a][b - 1]
                assert all(streamed[a][k - 1] >= cur for k in range(b + 1, b_max[a] + 1)), (a, got)


def test_round_by_round_order():
    rng = np.random.default_rng(11)
    for trial in range(300):
        A = int(rng.integers(1, 10))
        resident, streamed, b_max = shrinking_tables(rng, A, ties=trial % 2 == 0)
        own = int(rng.integers(0, 1 << 24))
        for avail in np.linspace(0, own + sum(resident), 9).astype(np.int64):
            sbv, need = prover.segment_stream_plan(resident, streamed, b_max, own, int(avail))
            check_round_order(resident, b_max, sbv)
            if need <= avail:
                assert need == planned_bytes(resident, streamed, own, sbv)


def test_fits_without_streaming_when_there_is_room():
    resident, streamed = [300, 200, 100], [[150, 100, 80, 70, 65]] * 3
    sbv, need = prover.segment_stream_plan(resident, streamed, [5, 5, 5], 10, 610)
    assert sbv == [0, 0, 0] and need == 610
    sbv, need = prover.segment_stream_plan(resident, streamed, [5, 5, 5], 10, 609)
    assert sbv == [1, 0, 0] and need == 460


def test_an_air_whose_streamed_size_is_not_smaller_is_skipped():
    # AIR 0 is the largest, but two sub-cosets would not make it smaller: round 1 passes it by and takes AIR 1; round 2 takes AIR 0
    resident = [1000, 800, 100]
    streamed = [[1000, 600, 500, 450, 420], [500, 300, 250, 220, 210], [90, 80, 70, 60, 55]]
    sbv, need = prover.segment_stream_plan(resident, streamed, [5, 5, 5], 0, 1700)
    assert sbv == [0, 1, 0] and need == 1600
    sbv, need = prover.segment_stream_plan(resident, streamed, [5, 5, 5], 0, 1200)
    assert sbv == [2, 1, 1] and need == 1190
    # a streamed size LARGER than the resident one is never taken, whatever the room
    sbv, need = prover.segment_stream_plan([100], [[200, 150, 120, 101, 100]], [5], 0, 0)
    assert sbv == [0] and need == 100


def test_each_airs_b_max_is_respected_and_nothing_more_helps():
    resident = [1000, 900, 800]
    streamed = [[500, 400, 300, 200, 100], [450, 350, 250, 150, 50], [400, 300, 200, 100, 10]]
    sbv, need = prover.segment_stream_plan(resident, streamed, [1, 5, 0], 7, 0)
    assert sbv == [1, 5, 0]
    assert need == 7 + 500 + 50 + 800 and need > 0
    sbv, need = prover.segment_stream_plan(resident, streamed, [3, 2, 4], 0, 0)
    assert sbv == [3, 2, 4] and need == 300 + 350 + 100
    # b_max 0 for all: the plan is the resident one, over the room
    sbv, need = prover.segment_stream_plan(resident, streamed, [0, 0, 0], 5, 100)
    assert sbv == [0, 0, 0] and need == 2705


def test_ties_keep_index_order():
    table = [[60, 50, 40, 30, 20]] * 4
    for avail, want in ((399, [1, 0, 0, 0]), (340, [1, 1, 0, 0]), (280, [1, 1, 1, 0]), (240, [1, 1, 1, 1]), (230, [2, 1, 1, 1])):
        sbv, _ = prover.segment_stream_plan([100] * 4, table, [5] * 4, 0, avail)
        assert sbv == want, (avail, sbv)
    # sizes 5, 9, 5, 9: the order is 1, 3, 0, 2
    resident = [500, 900, 500, 900]
    streamed = [[r // 2, r // 3, r // 4, r // 5, r // 6] for r in resident]
    steps = []
    for avail in range(2800, 0, -1):
        sbv, _ = prover.segment_stream_plan(resident, streamed, [5] * 4, 0, avail)
        if not steps or steps[-1] != sbv:
            steps.append(sbv)
    assert steps[:5] == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 1], [1, 1, 0, 1], [1, 1, 1, 1]]
    assert steps[5] == [1, 2, 1, 1]


def test_the_plan_only_grows_as_the_room_shrinks():
    rng = np.random.default_rng(23)
    for trial in range(150):
        A = int(rng.integers(1, 9))
        if trial % 2:
            resident, streamed, b_max = shrinking_tables(rng, A, ties=trial % 4 == 1)
        else:
            resident = [int(x) for x in rng.integers(1, 1000, A)]
            streamed = [[int(x) for x in rng.integers(1, 1200, 5)] for _ in range(A)]
            b_max = [int(x) for x in rng.integers(0, 6, A)]
        own = int(rng.integers(0, 1000))
        prev = None
        for avail in sorted(set(int(x) for x in rng.integers(0, own + sum(resident) + 1, 40)), reverse=True):
            sbv, _ = prover.segment_stream_plan(resident, streamed, b_max, own, avail)
            if prev is not None:
                assert {a for a, b in enumerate(prev) if b} <= {a for a, b in enumerate(sbv) if b}
                assert all(x >= y for x, y in zip(sbv, prev)), (prev, sbv)
            prev = sbv


@pytest.mark.parametrize("n", [0, 1])
def test_an_empty_or_single_air_table(n):
    sbv, need = prover.segment_stream_plan([64] * n, [[32, 16, 8, 4, 2]] * n, [5] * n, 3, 0)
    assert sbv == [5] * n and need == 3 + 2 * n
