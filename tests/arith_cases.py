"""Operand sets of the arithmetic-probe tests, shared by test_arith_emul.py (CPU emulation, loose=False) and test_arith_gpu.py (the
gfx950 assembly layer, loose=True).  Everything is deterministic: fixed seeds, no search that depends on the code under test.

Field operands are RAW limb values (Python integers): the device layer works in the loose domain [0, 2p), so the lists hold the
boundary values of that domain, values whose 32-bit limbs are all ones or a lone one (carry words), and seeded random values of both
halves.  loose=False keeps what lies in [0, p): in the emulation build the loose names are the strict host operations, and values at
or above p are outside their contract.

premises() checks -- from the reference alone -- that the lists really hold the cases the device layer can get wrong (a second fold,
a difference that is the representative p of zero, ...), so that a later edit of the lists cannot quietly make them easy."""
import random

import arith_ref as A
import pyref

M32 = 0xffffffff


def _dedupe(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v); out.append(v)
    return out


def edge_values(p, loose=True):
    """small and boundary values, the Montgomery constants, 2^(32k) - 1 / 2^(32k) / 2^(32k) + 1, the largest value below 2p whose seven
    low limbs are all ones, and every single-limb value 0xffffffff << 32k below 2p"""
    v = [0, 1, 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1, A.RMONT % p, A.RMONT * A.RMONT % p]
    for k in range(1, 8):
        v += [(1 << (32 * k)) - 1, 1 << (32 * k), (1 << (32 * k)) + 1]
    low7 = (1 << 224) - 1
    top = (2 * p - 1) >> 224
    v.append(((top << 224) | low7) if ((top << 224) | low7) < 2 * p else (((top - 1) << 224) | low7))
    v += [M32 << (32 * k) for k in range(8)]
    bound = 2 * p if loose else p
    return _dedupe([x for x in v if x < bound])


def random_values(p, n, seed, loose=True):
    """n seeded values: alternately from [0, p) and, in loose mode, from [p, 2p)"""
    rng = random.Random(seed)
    return [rng.randrange(p) + (p if loose and (i & 1) else 0) for i in range(n)]


N_RANDOM = 300          # random cases appended to every list
N_DRAWN = 400           # 4- and 8-operand tuples drawn from the edge list
N_NEAR_MAX = 1600       # near-maximal tuples (the block that reaches the second fold of lmul4)


def unary_cases(p, loose=True, seed=1):
    return [(v,) for v in edge_values(p, loose) + random_values(p, N_RANDOM, seed, loose)]


def binary_cases(p, loose=True, seed=2):
    """the full cross product of the edge list, plus random pairs"""
    e = edge_values(p, loose)
    r = random_values(p, 2 * N_RANDOM, seed, loose)
    return [(a, b) for a in e for b in e] + [(r[2 * i], r[2 * i + 1]) for i in range(N_RANDOM)] + [(r[2 * i], r[2 * i]) for i in range(8)]


def tuple_cases(p, width, neg_slots=(), loose=True, seed=3):
    """width = 4 or 8 operands.  Every all-equal edge tuple, tuples drawn from the edge list, random tuples, and a block of near-maximal
    tuples: operands 2p - 1 - j (p - 1 - j when not loose) with small j.  The slots in neg_slots are the ones the op passes through
    lneg_op (the operand becomes 2p - y): they are fed small y in that block, y = 0 included, which gives 2p itself."""
    rng = random.Random(seed * 1000 + width)
    e = edge_values(p, loose)
    out = [(v,) * width for v in e]
    out += [tuple(rng.choice(e) for _ in range(width)) for _ in range(N_DRAWN)]
    r = random_values(p, width * N_RANDOM, seed + 17, loose)
    out += [tuple(r[width * i:width * i + width]) for i in range(N_RANDOM)]
    top = (2 * p if loose else p) - 1
    for i in range(N_NEAR_MAX):
        t = []
        for s in range(width):
            j = 0 if i == 0 else rng.randrange(1 << (1 + i % 40))
            if s in neg_slots:
                t.append(j if loose else min(j, p - 1))          # y: the operand is 2p - y on the device
            else:
                t.append(top - min(j, top))
        out.append(tuple(t))
    return out


# name -> (probe index, operand words, result words, operand domain, case builder)
#   domain "strict": the primitive's contract is [0, p) operands (add, sub, neg); "loose": it takes [0, 2p)
FIELD_OPS = {
    "add": (0, 2, 1, "strict"), "sub": (1, 2, 1, "strict"), "neg": (2, 1, 1, "strict"), "mul": (3, 2, 1, "loose"),
    "reduce_once": (4, 1, 1, "loose"), "canon": (5, 1, 1, "loose"),
    "lmul": (6, 2, 1, "loose"), "lsqr": (7, 1, 1, "loose"), "ladd": (8, 2, 1, "loose"), "lsub": (9, 2, 1, "loose"),
    "ldbl": (10, 1, 1, "loose"), "lneg": (11, 1, 1, "loose"), "lis_zero": (12, 1, 1, "loose"),
    "lneg_op": (13, 1, 1, "loose"), "lmul_negop": (14, 2, 1, "loose"),
    "lmul2": (15, 4, 1, "loose"), "lmul2_negop": (16, 4, 1, "loose"), "lmul4": (17, 8, 1, "loose"), "lmul4_negop": (18, 8, 1, "loose"),
    "lmul_x2": (19, 4, 2, "loose"), "lmul2_x2": (20, 8, 2, "loose"),
    "to_mont": (21, 1, 1, "loose"), "from_mont": (22, 1, 1, "loose"), "inv": (23, 1, 1, "loose"),
}
STRICT_RESULT = ("add", "sub", "neg", "mul", "reduce_once", "canon", "to_mont", "from_mont", "inv")      # result in [0, p); the others in [0, 2p)
NEG_SLOTS = {"lmul_negop": (1,), "lmul2_negop": (3,), "lmul4_negop": (3, 7)}


def field_cases(name, p, loose=True):
    """the operand tuples (raw integers) of one field primitive"""
    _, width, _, domain = FIELD_OPS[name]
    lo = loose and domain == "loose"
    if name == "inv":                                     # 254 squarings per case: the edge list and a few random values
        return [(v,) for v in edge_values(p, lo) + random_values(p, 24, 5, lo)]
    if width == 1:
        return unary_cases(p, lo)
    if width == 2:
        return binary_cases(p, lo)
    return tuple_cases(p, width, NEG_SLOTS.get(name, ()), lo)


# ---- Fq2: elements are (c0, c1); the components run through the same lists
def fq2_cases(name, loose=True):
    q = A.FQ
    width = {"lmul": 2, "lsqr": 1, "lmul2": 4, "ladd": 2, "lsub": 2, "lis_zero": 1, "ldbl": 1, "lneg": 1, "canon": 1, "inv": 1, "eq": 2}[name]
    if name == "eq":                                      # every pair of representatives of every edge pair, near misses, and the drawn tuples
        e = edge_values(q, loose)
        pairs = [(a, b) for a in e for b in e if a % q == b % q or abs(a - b) in (1, q - 1, q + 1)]
        flat = [(a, c, b, d) for (a, b) in pairs for (c, d) in pairs[::7]] + tuple_cases(q, 4, (), loose, seed=12)[:N_DRAWN]
        return [((t[0], t[1]), (t[2], t[3])) for t in flat]
    if name == "inv":                                     # one Fq inversion per case: the edge cross product and a few random elements
        e = edge_values(q, loose)
        r = random_values(q, 48, 14, loose)
        return [((a, b),) for a in e[:12] for b in e[:12]] + [((r[2 * i], r[2 * i + 1]),) for i in range(24)]
    if name == "lis_zero":
        e = edge_values(q, loose)
        return [((a, b),) for a in e for b in e]
    flat = tuple_cases(q, 8, (), loose, seed=11) if width == 4 else tuple_cases(q, 4, (), loose, seed=12) if width == 2 else binary_cases(q, loose, seed=13)
    return [tuple((t[2 * i], t[2 * i + 1]) for i in range(width)) for t in flat]


FQ2_OPS = {"lmul": 0, "lsqr": 1, "lmul2": 2, "ladd": 3, "lsub": 4, "lis_zero": 5, "ldbl": 6, "lneg": 7, "canon": 8, "inv": 9, "eq": 10}
FQ2_FLAG = ("lis_zero", "eq")                             # result: 0 or 1 in the low limb of c0
FQ2_STRICT_RESULT = ("canon", "inv")                      # result in [0, q)


# ---- curves
CURVE_OPS = {"dbl_affine": 0, "dbl": 1, "madd": 2, "madd_pairs": 3, "add": 4, "dbl_q": 5, "add_q": 6, "madd_q": 7, "canon": 8, "to_affine": 9}
CURVE_SHAPE = {"dbl_affine": "A", "dbl": "X", "dbl_q": "X", "madd": "XA", "madd_pairs": "XA", "madd_q": "XA", "add": "XX", "add_q": "XX",
               "canon": "X", "to_affine": "X"}
SCALARS = [1, 2, 3, 0x1234567, A.FR - 1, A.FR - 2, 0x2b5a1d3f9c7e6b8a4d2f1e0c9b8a7d6e5f4c3b2a19081726354453627180f]


def curve_points(oracle, g2):
    """points of the order-r groups, canonical affine coordinates (pyref form): G1 from the oracle's batch_mul, G2 from pyref.g2_mul"""
    if g2:
        return [pyref.g2_mul(pyref.G2_GEN, k) for k in SCALARS]
    from ethsnarks_amd import fields as F
    pts = oracle.batch_mul(F.fr_to_mont(SCALARS))
    return [tuple(F.fq_from_mont(row.reshape(2, 4))) for row in pts]


class _CurveBuilder:
    def __init__(self, g2, loose, seed):
        self.g2, self.loose, self.rng, self.q = g2, loose, random.Random(seed), A.FQ
        self.ref = A.CurveRef(g2)

    def felem(self, nonzero=True):
        v = lambda: self.rng.randrange(1 if nonzero else 0, self.q)
        return (v(), v()) if self.g2 else v()

    def lams(self):
        q = self.q
        small = [1, 2, q - 1]
        return [((s, 0) if self.g2 else s) for s in small] + [self.felem(), self.felem()]

    def neg(self, P):
        return (P[0], pyref.f2_neg(P[1]) if self.g2 else (-P[1]) % self.q)

    def xyzz(self, P, lam):
        m = self.ref.mul
        l2 = m(lam, lam); l3 = m(l2, lam)
        return (m(P[0], l2), m(P[1], l3), l2, l3)

    def raw(self, coords, pattern):
        """canonical coordinate values -> raw Montgomery integers; bit i of `pattern` adds q to component i (loose mode only)"""
        out, i = [], 0
        for c in coords:
            comps = []
            for v in (c if self.g2 else (c,)):
                r = A.to_mont(self.q, v)
                if self.loose and (pattern >> i) & 1:
                    r += self.q
                comps.append(r); i += 1
            out.append(tuple(comps) if self.g2 else comps[0])
        return tuple(out)

    def patterns(self, k=3):
        """representative choices per coordinate: all canonical, all + q, and k random mixes (one choice in strict mode)"""
        if not self.loose:
            return [0]
        return [0, (1 << 16) - 1] + [self.rng.getrandbits(16) for _ in range(k)]

    def const(self, comps):
        """a coordinate whose components are the given raw values (G1: the first only)"""
        return tuple(comps[:2]) if self.g2 else comps[0]

    def infinities_x(self):
        """XYZZ infinity: all zero; ZZ = 0 with non-zero other coordinates; in loose mode ZZ = p with non-zero others, and mixes for G2"""
        q, z = self.q, self.const([0, 0])
        junk = lambda: self.raw((self.felem(), self.felem(), self.felem()), self.rng.getrandbits(8) if self.loose else 0)
        out = [(z, z, z, z)]
        j = junk(); out.append((j[0], j[1], z, j[2]))
        if self.loose:
            j = junk(); out.append((j[0], j[1], self.const([q, q]), j[2]))
            if self.g2:
                j = junk(); out.append((j[0], j[1], self.const([0, q]), j[2]))
                j = junk(); out.append((j[0], j[1], self.const([q, 0]), j[2]))
        return out

    def infinities_a(self):
        """affine infinity: (0, 0); in loose mode also (p, p), (0, p), (p, 0) (G2: the same choice in every component, and two mixes)"""
        q = self.q
        c = lambda a, b: self.const([a, b])
        out = [(c(0, 0), c(0, 0))]
        if self.loose:
            out += [(c(q, q), c(q, q)), (c(0, 0), c(q, q)), (c(q, q), c(0, 0))]
            if self.g2:
                out += [(c(0, q), c(q, 0)), (c(q, 0), c(0, q))]
        return out


def curve_cases(name, points, g2, loose=True):
    """[(label, operands)]: operands are tuples of raw Montgomery coordinates, affine (x, y) or XYZZ (X, Y, ZZ, ZZZ)"""
    b = _CurveBuilder(g2, loose, seed=100 + CURVE_OPS[name] + (50 if g2 else 0))
    shape = CURVE_SHAPE[name]
    lams = b.lams()
    cases = []
    X = lambda P, lam, pat: b.raw(b.xyzz(P, lam), pat)
    Af = lambda P, pat: b.raw(P, pat)
    if shape == "A":
        for i, P in enumerate(points):
            for pat in b.patterns():
                cases.append(("2P affine #%d" % i, (Af(P, pat),)))
        cases += [("affine infinity", (a,)) for a in b.infinities_a()]
    elif shape == "X":
        for i, P in enumerate(points):
            for lam in lams:
                for pat in b.patterns(2):
                    cases.append(("P #%d" % i, (X(P, lam, pat),)))
        cases += [("infinity", (x,)) for x in b.infinities_x()]
    elif shape == "XA":
        n = len(points)
        for i in range(n):
            P, Q = points[i], points[(i + 1) % n]
            for lam in lams:
                for pat in b.patterns(2):
                    cases.append(("P + Q", (X(P, lam, pat), Af(Q, pat >> 8))))
                    cases.append(("P + P", (X(P, lam, pat), Af(P, pat >> 8))))
                    cases.append(("P + (-P)", (X(P, lam, pat), Af(b.neg(P), pat >> 8))))
            one = (1, 0) if g2 else 1
            for pat in b.patterns(2):
                cases.append(("(x, y, 1, 1) + P", (X(P, one, pat), Af(P, pat >> 8))))
        for x in b.infinities_x():
            for pat in b.patterns(1):
                cases.append(("infinity + Q", (x, Af(points[2], pat))))
            for a in b.infinities_a():
                cases.append(("infinity + infinity", (x, a)))
        for a in b.infinities_a():
            for pat in b.patterns(1):
                cases.append(("P + infinity", (X(points[3], lams[3], pat), a)))
    elif shape == "XX":
        n = len(points)
        for i in range(n):
            P, Q = points[i], points[(i + 2) % n]
            for k, lam in enumerate(lams):
                mu = lams[(k + 1) % len(lams)]                 # the other side's Z: always a different one
                for pat in b.patterns(2):
                    cases.append(("P + Q", (X(P, lam, pat), X(Q, mu, pat >> 8))))
                    cases.append(("P + P, different Z", (X(P, lam, pat), X(P, mu, pat >> 8))))
                    cases.append(("P + (-P), different Z", (X(P, lam, pat), X(b.neg(P), mu, pat >> 8))))
            cases.append(("P + P, same limbs", (X(P, lams[3], 0), X(P, lams[3], 0))))
        for x in b.infinities_x():
            for pat in b.patterns(1):
                cases.append(("infinity + Q", (x, X(points[2], lams[4], pat))))
                cases.append(("P + infinity", (X(points[3], lams[3], pat), x)))
            for y in b.infinities_x():
                cases.append(("infinity + infinity", (x, y)))
    return cases


# ---- premises: the lists hold the hard cases (reference only, no code under test involved)
def premises(p):
    two_p = 2 * p
    for name in ("lmul2", "lmul2_negop"):
        cls = {A.dot_exact(p, t, NEG_SLOTS.get(name, ())) >= two_p for t in field_cases(name, p)}
        assert cls == {False, True}, (name, cls)
    for name in ("lmul4", "lmul4_negop"):
        cls = {min(A.dot_exact(p, t, NEG_SLOTS.get(name, ())) // two_p, 2) for t in field_cases(name, p)}
        assert cls == {0, 1, 2}, (name, cls)                       # < 2p, [2p, 4p), >= 4p: no fold, one, two
    halves = {min(A.dot_exact(p, t[4 * h:4 * h + 4]) // two_p, 1) for t in field_cases("lmul2_x2", p) for h in (0, 1)}
    assert halves == {0, 1}
    diffs = {a - b for a, b in field_cases("lsub", p)}
    assert {0, p, two_p - 1, -p} <= diffs, "lsub: differences 0, p, 2p - 1 and -p (the result is the representative p of zero)"
    assert any(two_p <= a + b < 2 * two_p for a, b in field_cases("ladd", p))
    assert any(a + b == two_p for a, b in field_cases("ladd", p)) and any(a + b == p for a, b in field_cases("ladd", p))
    assert {0, p, 1, p - 1, p + 1, two_p - 1} <= {t[0] for t in field_cases("lis_zero", p)}
    assert any(t[0] == 0 for t in field_cases("lneg_op", p)) and any(t[3] == 0 for t in field_cases("lmul2_negop", p))   # lneg_op gives 2p itself
    for name in FIELD_OPS:                                        # operands stay inside each primitive's contract
        bound = two_p if FIELD_OPS[name][3] == "loose" else p
        slots = NEG_SLOTS.get(name, ())
        assert all(v < bound for t in field_cases(name, p) for i, v in enumerate(t) if i not in slots), name
        assert all(v < p for name2 in (name,) for t in field_cases(name2, p, loose=False) for v in t), name
