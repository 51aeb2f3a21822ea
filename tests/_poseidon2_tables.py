"""Round-constant tables that are extreme where the rounds of the signed Poseidon2 (csrc/poseidon2.hpp) consume them.

The rounds do not read ext_rc / int_rc but the tables derive_params folds them into: per external round r != 4 and block q the
seeds and corrections (a, b, d1, d3) of the M4 network, f = c - colsum / 5, a = (2 f0 - f2) / 3, b = (2 f2 - f0) / 3, d1 = f1 - a - b,
d3 = f3 - a - b, all times the scale of the layer's inputs; int_rc[0] as entry_c; int_rc[1..12] and ext_rc[4][0] as int_fold;
ext_rc[4][1..15] as exit_fold. The range analysis (tools/poseidon2_bounds.py) lets every one of them sit at +-(p - 1) / 2 at once;
raw tables of equal words fold to small multiples of c / 15. The map raw -> folded is linear and invertible per round, so
table_for_folded inverts it: plain Python integers, the scales restated from the comments in Params."""
import random

P = 0x78000001
R = (1 << 32) % P
HALF = (P - 1) // 2


def _inv(x):
    return pow(x % P, P - 2, P)


def _centred(x):
    x %= P
    return x - P if x > P // 2 else x


def scales():
    """(scale of the inputs of the layer that precedes external round r, for r = 0..7; first-half scale; second-half scale):
    a register at scale lam holds lam * (Montgomery word). Layer 0 sees scale 1 and divides by R; x -> x^7 raises the scale to
    its 7th power; every layer but the last divides by R; the last layer must see scale 1."""
    rinv, d7 = _inv(R), pow(7, -1, P - 1)
    a = [0] * 8  # scale at the input of the S-box of external round r
    a[0] = rinv
    for r in range(1, 4):
        a[r] = pow(a[r - 1], 7, P) * rinv % P
    lam_first = pow(a[3], 7, P) * rinv % P
    a[7] = 1
    for r in (6, 5, 4):
        a[r] = pow(R * a[r + 1] % P, d7, P)
    layer_in = [1] + [pow(a[r - 1], 7, P) for r in range(1, 8)]
    return layer_in, lam_first, a[4]


def table_for_folded(targets):
    """targets = dict(ext_fold=8 x 16 (row 4 is not free: zeros), entry_c, int_fold=13, exit_fold=16 ([0] is not free: zero)): the
    centred values the rounds shall consume (int_fold / exit_fold: the centred factor of R mod p). Returns (ext_rc 8 x 16, int_rc 13)
    as canonical words."""
    layer_in, lam_first, lam_second = scales()
    rinv = _inv(R)
    ext = [[0] * 16 for _ in range(8)]  # Montgomery words first
    for r in range(8):
        if r == 4:
            continue
        li = _inv(layer_in[r])
        f = [0] * 16
        for q in range(4):
            a, b, d1, d3 = (t * li % P for t in targets["ext_fold"][r][4 * q:4 * q + 4])
            f[4 * q:4 * q + 4] = [(2 * a + b) % P, (d1 + a + b) % P, (a + 2 * b) % P, (d3 + a + b) % P]
        for i in range(4):
            col = sum(f[4 * q + i] for q in range(4))
            for q in range(4):
                ext[r][4 * q + i] = (f[4 * q + i] + col) % P
    l2 = _inv(lam_second)
    ext[4][0] = targets["int_fold"][12] * l2 % P
    for i in range(1, 16):
        ext[4][i] = targets["exit_fold"][i] * l2 % P
    intr = [targets["entry_c"] * _inv(lam_first) % P] + [targets["int_fold"][r] * l2 % P for r in range(12)]
    return [[w * rinv % P for w in row] for row in ext], [w * rinv % P for w in intr]


def expected_derived(targets, diag_canonical):
    """What powdr_poseidon2_derived must return for table_for_folded(targets) (prover.poseidon2_derived's layout); part_* depend on
    the scales and the internal diagonal only."""
    _, lam_first, lam_second = scales()
    out = dict(ext_fold=[[0] * 16 if r == 4 else list(targets["ext_fold"][r]) for r in range(8)], entry_c=targets["entry_c"],
               int_fold=[t * R for t in targets["int_fold"]], exit_fold=[0] + [t * R for t in targets["exit_fold"][1:]],
               part_kappa=[], part_rho=[], part_diag=[])
    for lin in (lam_first, lam_second):
        l0 = pow(lin, 7, P)
        ratio, ratio0 = lam_second * _inv(lin) % P, lam_second * _inv(l0) % P
        out["part_kappa"].append(_centred(lin * _inv(l0)))
        out["part_rho"].append(_centred(ratio * R * R))
        out["part_diag"].append([_centred(d * R * (ratio if i else ratio0)) for i, d in enumerate(int(x) for x in diag_canonical)])
    return out


def _targets(sign):
    """sign(kind, round, index) -> a centred value; kind 'ext' (round 0..7), 'int' (entry_c: round 0, int_fold[r]: round r + 1),
    'exit' (round 4)"""
    return dict(ext_fold=[[0 if r == 4 else sign("ext", r, i) for i in range(16)] for r in range(8)], entry_c=sign("int", 0, 0),
                int_fold=[sign("int", r + 1, 0) for r in range(13)], exit_fold=[0] + [sign("exit", 4, i) for i in range(1, 16)])


def named_targets():
    rng = random.Random(0x9053)
    return [("plus_half", _targets(lambda k, r, i: HALF)),
            ("minus_half", _targets(lambda k, r, i: -HALF)),
            ("alternating_by_word", _targets(lambda k, r, i: -HALF if i & 1 else HALF)),
            ("alternating_by_round", _targets(lambda k, r, i: -HALF if r & 1 else HALF)),
            ("random_0", _targets(lambda k, r, i: rng.randint(-HALF, HALF))),
            ("random_1", _targets(lambda k, r, i: rng.randint(-HALF, HALF)))]


def named_tables():
    """[(name, targets, ext_rc, int_rc)]: every folded constant at +HALF, at -HALF, alternating by word, by round, two random ones"""
    import numpy as np

    out = []
    for name, t in named_targets():
        e, i = table_for_folded(t)
        out.append((name, t, np.array(e, np.uint32), np.array(i, np.uint32)))
    return out


def edge_matrices(height, W):
    """{kind: column-major [W * height] canonical matrix}: all 0, all p - 1, column c = (p -+ 1) / 2 alternating by column, one-hot
    rows, random — the words a leaf hash absorbs at the edges of the field"""
    import numpy as np

    rng = np.random.default_rng(1000 * W + height)
    halves = np.array([(P - 1) // 2, (P + 1) // 2], np.uint32)
    one_hot = np.zeros((W, height), np.uint32)
    one_hot[np.arange(height) % W, np.arange(height)] = np.where(np.arange(height) % 2, P - 1, 1)
    return {"zeros": np.zeros(W * height, np.uint32), "p_minus_1": np.full(W * height, P - 1, np.uint32),
            "halves_by_column": np.repeat(halves[np.arange(W) % 2], height), "one_hot_rows": one_hot.reshape(-1),
            "random": rng.integers(0, P, W * height, dtype=np.uint32)}
