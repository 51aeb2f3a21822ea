"""Exact value ranges of the signed extension arithmetic (bb::sfold / smont_any in powdr_amd/csrc/babybear.hpp, bb::SExt and its
operations in csrc/ext.hpp, the LogUp helpers of csrc/jit_device.hpp).  Every 32-bit word must fit an int32, every 64-bit sum an
int64, every argument of the plain signed Montgomery reduction must satisfy |t| + 2^31 p <= 2^63 - 1.  All bounds are INCLUSIVE
maxima of magnitudes.  The ranges close from three kinds of input: canonical words centred on load (|x| <= (p - 1) / 2), centred
wave-uniform challenges (the same), and outputs of smont / smont_any.
The figures are kept as exact integers in the blocks "namespace bounds" of babybear.hpp and ext.hpp; this tool reads both blocks
from the header text and asserts every constant against what it computes (tests/test_ext_signed_bounds.py runs it)."""
import re
from pathlib import Path

p, R = 0x78000001, 1 << 32
KAPPA = R % p                 # Montgomery 1
W11R = 11 * R % p             # Montgomery 11
I32, I64MAX = 1 << 31, (1 << 63) - 1
HALF = (p - 1) // 2           # largest centred representative
assert KAPPA <= HALF and W11R <= HALF, "both constants are centred as they stand"
SMONT_DOMAIN = I64MAX - I32 * p


def smont(tmax):
    """|t| <= tmax -> max |(t + m p) >> 32| for a signed m in [-2^31, 2^31)"""
    assert tmax <= SMONT_DOMAIN, f"|t| = {tmax / p / p:.4f} p^2 leaves the domain of the signed reduction"
    out = (tmax + I32 * p) >> 32
    assert out < I32
    return out


def fits(tmax, what):
    assert tmax <= I64MAX, f"{what}: {tmax / p / p:.4f} p^2 does not fit an int64 ({I64MAX / p / p:.4f} p^2)"
    return tmax


# ---- the fold: T = Th 2^32 + Tl -> Th kappa + Tl, Th in [-2^31, 2^31), Tl in [0, 2^32)
SFOLD = max(I32 * KAPPA, (I32 - 1) * KAPPA + R - 1)
S = smont(SFOLD)              # class S: outputs of smont_any, whatever int64 went in
assert HALF <= S
print(f"sfold: |T'| <= {SFOLD / p / p:.5f} p^2; smont_any: |x| <= {S / p:.5f} p (class S)")

# ---- extension product a b: a in class W (or S), b in class S with b1..b3 pre-multiplied by 11 (plain smont: one-term products)
PRE = smont(S * W11R)
WIDE = smont(2 * S * HALF)    # class W: scale2 (two S x centred products in one plain reduction)
SCALE = smont(S * HALF)       # scale by a centred base word
assert WIDE < p and SCALE < p, "canonical_of_centred takes (-p, p)"
ADDEND = max(S * HALF, WIDE * KAPPA, HALF * KAPPA)   # the fifth term of mul_add_scaled / mul_sub / mul_sub_base
MULSUM = fits(4 * WIDE * max(S, PRE) + ADDEND, "a coordinate of the extension product")
print(f"product: 11 b <= {PRE / p:.5f} p, class W <= {WIDE / p:.5f} p, coordinate sums <= {MULSUM / p / p:.4f} p^2 of {I64MAX / p / p:.4f} p^2")
MULSUB2 = fits(4 * HALF * max(S, PRE) + 2 * S * HALF, "sext_mul_sub_scaled2")
# how wide could the first operand be at all (for the record)
amax = (I64MAX - ADDEND) // (4 * max(S, PRE))
print(f"product: the first operand may be as wide as {amax / p:.4f} p")

# ---- inverse: d0 = a0^2 + 11 a2^2 - 22 a1 a3, d1 = 2 a0 a2 - a1^2 - 11 a3^2 (four products each), n = d0^2 - 11 d1^2
fits(4 * S * max(S, PRE), "d0 / d1 of ext_inv_prepare")
NORMSUM = S * S + S * PRE
NORM = smont(NORMSUM)
CHAIN = max(NORM, KAPPA)      # the inversion chain: products of two chain words, plain smont
while smont(CHAIN * CHAIN) > CHAIN:
    CHAIN = smont(CHAIN * CHAIN)
assert smont(CHAIN * CHAIN) <= CHAIN
E = smont(S * CHAIN)          # d0 / n, -d1 / n
E11 = smont(E * W11R)
fits(2 * S * max(E, E11), "a coordinate of ext_inv_finish")
print(f"inverse: |n| <= {NORM / p:.5f} p, the chain closes at {CHAIN / p:.5f} p (products {CHAIN * CHAIN / p / p:.4f} p^2 of {SMONT_DOMAIN / p / p:.4f} p^2), "
      f"|e| <= {E / p:.5f} p, |11 e| <= {E11 / p:.5f} p")

# ---- accumulators
DENSEED = HALF * KAPPA
assert DENSEED <= SFOLD
DENTERM = (p - 1) * HALF      # a canonical argument times a centred challenge coordinate
DEN_TERMS = (I64MAX - SFOLD) // DENTERM
CENTERM = HALF * HALF         # ExtCentredAcc: both centred
CEN_TERMS = (I64MAX - SFOLD) // CENTERM
ACCTERM = HALF * S            # SExtProductAcc: a centred challenge coordinate times a class-S word; coefficient k has min(k+1, 7-k) of them
ACC_PERIOD = [(I64MAX - SFOLD) // (c * ACCTERM) for c in (1, 2, 3, 4)]
assert DEN_TERMS >= 1 and min(ACC_PERIOD) >= 1
ACC_H = smont(SFOLD)
ACC_OUT = smont(SFOLD + ACC_H * W11R)
assert ACC_OUT < p
print(f"denominator: {DEN_TERMS} terms between folds; centred sums: {CEN_TERMS}; product accumulator: a fold every {ACC_PERIOD} terms "
      f"(coefficients 0/6, 1/5, 2/4, 3), result |x| <= {ACC_OUT / p:.5f} p")

computed = {
    "kSmontDomain": SMONT_DOMAIN, "kSfoldMax": SFOLD, "kSmontAnyMax": S,
    "kHalf": HALF, "kPre11Max": PRE, "kWideMax": WIDE, "kScaleMax": SCALE, "kMulAddendMax": ADDEND, "kMulSumMax": MULSUM, "kMulSub2SumMax": MULSUB2,
    "kNormSumMax": NORMSUM, "kNormMax": NORM, "kChainMax": CHAIN, "kInvEMax": E, "kInvE11Max": E11,
    "kDenTerm": DENTERM, "kDenTermsPerFold": DEN_TERMS, "kCentredTermsPerFold": CEN_TERMS,
    "kAccTerm": ACCTERM, "kAccPeriod0": ACC_PERIOD[0], "kAccPeriod1": ACC_PERIOD[1], "kAccPeriod2": ACC_PERIOD[2], "kAccPeriod3": ACC_PERIOD[3],
    "kAccOutMax": ACC_OUT,
}


def stated_bounds():
    csrc = Path(__file__).resolve().parents[1] / "powdr_amd" / "csrc"
    stated = {}
    for name in ("babybear.hpp", "ext.hpp"):
        block = re.search(r"namespace bounds \{(.*?)\}  // namespace bounds", (csrc / name).read_text(), flags=re.S)
        assert block, f"{name} has no bounds block"
        for m in re.finditer(r"constexpr int(?:32|64)_t (k\w+) = (-?\d+)(?:ll)?;", block.group(1)):
            assert m.group(1) not in stated, m.group(1)
            stated[m.group(1)] = int(m.group(2))
    return stated


def check():
    stated = stated_bounds()
    assert set(stated) == set(computed), sorted(set(stated) ^ set(computed))
    for name, want in computed.items():
        assert stated[name] == want, f"the headers state {name} = {stated[name]}, computed {want}"
    return len(stated)


if __name__ == "__main__":
    for name, v in computed.items():
        print(f"  {name} = {v}")
    print(f"babybear.hpp / ext.hpp bounds: {check()} constants agree")
