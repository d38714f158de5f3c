"""Operand lists and checks for the lazy Karatsuba Fq2 product (csrc/bn254.hpp, Field::lmul_k / lmul2_k behind Fq2::lmul / lmul2), shared
by test_fq2_karatsuba_emul.py and test_fq2_karatsuba_gpu.py.  Both run the SAME lists through the arithmetic probe (ZK_PROBE_FQ2 ops 0 and
2): the emulation build computes the algorithm in plain C++, the device in the gfx950 assembly layer.

Every component of every operand comes from EDGE = {0, 1, q-1, q, q+1, 2q-1}, the loose domain [0, 2q) with its upper edge:
  * lmul: all 6^4 = 1296 combinations of (a0, a1, b0, b1).
  * lmul2 (a b + c d): the two products enter the columns symmetrically and share nothing but the final sums, so the list pairs each of the
    1296 (a, b) with the (c, d) at three strides coprime to 1296 (every component sees every edge value in both products, and every (a, b)
    meets three different (c, d)) instead of the 6^8 full product, which no quick test can run.
  * the two extremes of c0's difference v0 - v1, explicitly: most negative a0 = b0 = 0, a1 = b1 = 2q-1 (the difference wraps and takes
    the masked addition), most positive a0 = b0 = 2q-1, a1 = b1 = 0 -- for lmul2 in both products at once.
  * 300 seeded random loose values per form.
The contract is the loose one: both result components equal the big-int value mod q (i.e. after canon) and lie below 2q."""
import itertools
import random
import arith_ref as A
import arith_checks as chk
import arith_cases as K

Q = A.FQ
EDGE = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1]
_E2 = [(x, y) for x in EDGE for y in EDGE]
LMUL_EDGE = [(a, b) for a in _E2 for b in _E2]                       # 1296
NEG = ((0, 2 * Q - 1), (0, 2 * Q - 1))                               # v0 - v1 = -(2q-1)^2
POS = ((2 * Q - 1, 0), (2 * Q - 1, 0))                               # v0 - v1 = +(2q-1)^2


def _rand(n, width, seed):
    rng = random.Random(seed)
    return [tuple((rng.randrange(2 * Q), rng.randrange(2 * Q)) for _ in range(width)) for _ in range(n)]


def lmul_cases():
    return [NEG, POS] + LMUL_EDGE + _rand(300, 2, 20251)


def lmul2_cases():
    n = len(LMUL_EDGE)
    out = [NEG + NEG, POS + POS, NEG + POS, POS + NEG]
    for stride, shift in ((1, 0), (5, 7), (625, 11)):                # all coprime to 1296 = 2^4 3^4
        out += [LMUL_EDGE[i] + LMUL_EDGE[(i * stride + shift) % n] for i in range(n)]
    return out + _rand(300, 4, 20252)


def premises():
    """from the lists alone: the edge set reaches every input slot, and both extremes of v0 - v1 are there"""
    for cases, width in ((lmul_cases(), 2), (lmul2_cases(), 4)):
        for slot in range(width):
            for comp in range(2):
                assert {t[slot][comp] for t in cases} >= set(EDGE)
        d = [sum(t[k][0] * t[k + 1][0] - t[k][1] * t[k + 1][1] for k in range(0, width, 2)) for t in cases]
        assert min(d) == -(width // 2) * (2 * Q - 1) ** 2 and max(d) == (width // 2) * (2 * Q - 1) ** 2


def check(zk, name):
    cases = {"lmul": lmul_cases, "lmul2": lmul2_cases}[name]()
    width = len(cases[0])
    got = chk._probe(zk, zk.PROBE_FQ2 + K.FQ2_OPS[name], [c for t in cases for e in t for c in e], 2 * width)
    bad = []
    for i, (t, g) in enumerate(zip(cases, got)):
        exp = A.fq2_expected(name, t)
        if (g[0] % Q, g[1] % Q) != exp or g[0] >= 2 * Q or g[1] >= 2 * Q:
            bad.append("fq2 %s case %d operands %s: got %s, want %s (mod q) below 2q" % (name, i, chk._hx(t), chk._hx(tuple(g)), chk._hx(exp)))
    chk._report("fq2 %s, Karatsuba operand list (%d cases)" % (name, len(cases)), bad)
