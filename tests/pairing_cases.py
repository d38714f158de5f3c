"""Operand lists of the pairing-probe tests, shared by test_pairing_emul.py (CPU emulation, loose=False: operands below q) and
test_pairing_gpu.py (the device tower in the loose domain [0, 2q), loose=True).  Everything is deterministic: fixed seeds, no search that
depends on the code under test.

Operands are RAW limb values (Python integers), Montgomery form: a raw value v stands for v 2^-256 mod q.  An fe12 is 12 words in the
order of zk_pairing_tower_op, an fe6 the first 6 of them.  premises() asserts -- from the reference alone -- that every kind of hard
case is present, so that a later edit of the lists cannot quietly make them easy."""
import functools
import random

import pyref
import verify_batch_cases as V

Q, R = pyref.Q, pyref.R
RM = 1 << 256
RINV = pow(RM, -1, Q)
ONE = RM % Q                                              # Montgomery form of 1
EASY_POWER = (Q ** 6 - 1) * (Q ** 2 + 1)
# name -> index of include/zkhip.h's zk_pairing_probe table
OPS = {"f6mul": 0, "f6mul_alias": 1, "f6mul01": 2, "f6inv": 3, "f6mulv": 4, "f6add": 5, "f6sub": 6, "f6neg": 7, "f2mulxi": 8, "f2muls": 9,
       "f2conj": 10, "f12mul": 11, "f12mul_alias": 12, "f12sqr": 13, "f12sqr_alias": 14, "f12inv": 15, "f12inv_alias": 16, "f12conj": 17,
       "f12frob1": 18, "f12frob2": 19, "f12frob3": 20, "f12cycsqr": 21, "f12cycsqr_alias": 22, "f12mul034": 23, "f12eq": 24, "f12is_one": 25,
       "f12canon": 26, "f12exp_negz": 27, "final_exp_easy": 28, "final_exp": 29, "dbl_step": 30, "add_step": 31, "g2_frob1": 32,
       "g2_negfrob2": 33, "ell": 34, "miller1": 35, "miller2": 36, "miller3": 37, "miller_fixed1": 38, "miller_fixed2": 39,
       "pair_product1": 40, "pair_product2": 41, "pair_product3": 42, "g2_on_curve": 43, "g2_in_subgroup": 44, "g1_on_curve": 45}
SHAPES = {"f6mul": (12, 6), "f6mul_alias": (12, 6), "f6mul01": (10, 6), "f6inv": (6, 6), "f6mulv": (6, 6), "f6add": (12, 6), "f6sub": (12, 6),
          "f6neg": (6, 6), "f2mulxi": (2, 2), "f2muls": (3, 2), "f2conj": (2, 2), "f12mul": (24, 12), "f12mul_alias": (24, 12), "f12sqr": (12, 12),
          "f12sqr_alias": (12, 12), "f12inv": (12, 12), "f12inv_alias": (12, 12), "f12conj": (12, 12), "f12frob1": (12, 12), "f12frob2": (12, 12),
          "f12frob3": (12, 12), "f12cycsqr": (12, 12), "f12cycsqr_alias": (12, 12), "f12mul034": (18, 12), "f12eq": (24, 1), "f12is_one": (12, 1),
          "f12canon": (12, 12), "f12exp_negz": (12, 12), "final_exp_easy": (12, 12), "final_exp": (12, 12), "dbl_step": (6, 12),
          "add_step": (10, 12), "g2_frob1": (4, 4), "g2_negfrob2": (4, 4), "ell": (21, 12), "miller1": (6, 12), "miller2": (12, 12),
          "miller3": (18, 12), "miller_fixed1": (7, 12), "miller_fixed2": (13, 12), "pair_product1": (6, 12), "pair_product2": (12, 12),
          "pair_product3": (18, 12), "g2_on_curve": (4, 1), "g2_in_subgroup": (4, 1), "g1_on_curve": (2, 1)}
STRICT_RESULT = ("f12canon", "pair_product1", "pair_product2", "pair_product3")     # documented strict: every word < q


def mont(v):
    return v * RM % Q


def dm(v):
    return v * RINV % Q


def edge_values(loose):
    """the coefficient edges of the loose domain: 0, 1 R, q - 1, q, q + 1, 2q - 1, (R mod q) + q"""
    return [v for v in (0, ONE, Q - 1, Q, Q + 1, 2 * Q - 1, ONE + Q) if loose or v < Q]


def raw(vals, rng, loose):
    """canonical values -> raw Montgomery words, in loose mode each with q added at random"""
    return [mont(v) + (Q if loose and rng.getrandbits(1) else 0) for v in vals]


def rand_words(rng, n, loose):
    return [rng.randrange(2 * Q if loose else Q) for _ in range(n)]


def elements(width, loose, seed, n_drawn=10, n_random=6):
    """[(label, words)]: elements of `width` coefficients (12: Fq12, 6: Fq6, 2: Fq2) on the edges of the domain"""
    rng = random.Random(seed)
    e = edge_values(loose)
    out = [("all %#x.." % (v >> 224), [v] * width) for v in e]               # all at q: loose zero; all at 2q - 1; all at 0 ...
    out.append(("one", [ONE] + [0] * (width - 1)))
    if loose:
        out.append(("loose one", [ONE + Q] + [Q] * (width - 1)))
        out.append(("loose one, mixed zeros", [ONE + Q] + [Q if i & 1 else 0 for i in range(width - 1)]))
    out += [("edge draw %d" % i, [rng.choice(e) for _ in range(width)]) for i in range(n_drawn)]
    out += [("random %d" % i, rand_words(rng, width, loose)) for i in range(n_random)]
    return out


def negated(words, rng, loose, add=None):
    """-a in a representative of its own: (-a mod q), plus q at random in loose mode (add: for every word or for none)"""
    out = []
    for w in words:
        v = (-w) % Q
        out.append(v + (Q if loose and (rng.getrandbits(1) if add is None else add) else 0))
    return out


# ---------------------------------------------------------------- the tower
def f6_pairs(loose):
    rng = random.Random(601)
    el = elements(6, loose, 600)
    out = [(la + " x " + lb, a + b) for (la, a), (lb, b) in zip(el, el[3:] + el[:3])]
    out += [(la + " squared", a + a) for la, a in el[:6]]
    for i in range(4):                                     # Karatsuba sums that vanish: a.c1 = -a.c0, a.c2 = -a.c0 (either representative of zero)
        a0 = rand_words(rng, 2, loose)
        a = a0 + negated(a0, rng, loose, add=False) + negated(a0, rng, loose, add=True)
        out.append(("c1 = c2 = -c0 #%d" % i, a + rand_words(rng, 6, loose)))
        out.append(("both c1 = c2 = -c0 #%d" % i, a + a))
    return out


def f12_pairs(loose):
    rng = random.Random(1201)
    el = elements(12, loose, 1200)
    out = [(la + " x " + lb, a + b) for (la, a), (lb, b) in zip(el, el[5:] + el[:5])]
    for i in range(4):
        a0 = rand_words(rng, 6, loose)
        a = a0 + negated(a0, rng, loose, add=bool(i & 1))
        b = rand_words(rng, 12, loose)
        out.append(("a.c0 = -a.c1 #%d" % i, a + b))
        out.append(("a.c0 = -a.c1, b likewise #%d" % i, a + b[:6] + negated(b[:6], rng, loose)))
        out.append(("a.c1 = 0 #%d" % i, a0 + [Q if loose and (i & 1) else 0] * 6 + b))
    for i in range(4):                                     # b sparse in the 0-3-4 pattern (the dense product must agree with f12mul034)
        out.append(("b sparse 0-3-4 #%d" % i, rand_words(rng, 12, loose) + sparse034(rand_words(rng, 6, loose), loose and i & 1)))
    return out


def sparse034(six, loose_zero=False):
    """(c0, d0, d1) as six words -> the fe12 c0 + (d0 + d1 v) w"""
    z = Q if loose_zero else 0
    return six[0:2] + [z] * 4 + six[2:6] + [z] * 2


def mul034_cases(loose):
    rng = random.Random(341)
    el = elements(12, loose, 340, n_drawn=6, n_random=4)
    e = edge_values(loose)
    out = []
    for i, (la, a) in enumerate(el):
        line = [rng.choice(e) for _ in range(6)] if i % 3 == 0 else rand_words(rng, 6, loose)
        if i % 5 == 1:
            line[2 * (i % 3):2 * (i % 3) + 2] = [Q if loose else 0, 0]          # a line with a vanishing coefficient
        out.append((la, a + line))
    out.append(("the line 1", el[-1][1] + [ONE, 0, 0, 0, 0, 0]))
    return out


def f12_unary(loose):
    rng = random.Random(1301)
    out = elements(12, loose, 1300)
    for i in range(3):
        a0 = rand_words(rng, 6, loose)
        out.append(("c0 = -c1 #%d" % i, a0 + negated(a0, rng, loose)))
        out.append(("c1 = 0 #%d" % i, a0 + [0] * 6))
        out.append(("c0 = 0 #%d" % i, [Q if loose else 0] * 6 + a0))
    return out


def f6_unary(loose):
    rng = random.Random(611)
    out = elements(6, loose, 610)
    for i in range(3):                                     # two zero coefficients (either representative)
        z = [Q if loose and i == 1 else 0] * 2
        c = rand_words(rng, 2, loose)
        out += [("only c0 #%d" % i, c + z + z), ("only c1 #%d" % i, z + c + z), ("only c2 #%d" % i, z + z + c)]
    return out


def basis_elements():
    out = []
    for k in range(12):
        w = [0] * 12
        w[k] = ONE
        out.append(("basis %d" % k, w))
    return out


def frob_cases(loose):
    rng = random.Random(1401)
    out = basis_elements()
    out += [("random %d" % i, rand_words(rng, 12, loose)) for i in range(3)]
    e = edge_values(loose)
    out += [("edge draw %d" % i, [rng.choice(e) for _ in range(12)]) for i in range(3)]
    out.append(("top", [(2 * Q if loose else Q) - 1] * 12))
    return out


@functools.lru_cache(maxsize=None)
def cyclotomic_values():
    """three elements of the cyclotomic subgroup, canonical tower coefficients: final_exp_easy of random elements, by the reference"""
    rng = random.Random(77)
    out = []
    for _ in range(3):
        a = [rng.randrange(Q) for _ in range(12)]
        g = pyref.f12_pow(V.tower_to_pyref(a), EASY_POWER)
        out.append(pyref_to_tower(g))
    return out


def pyref_to_tower(p):
    """inverse of verify_batch_cases.tower_to_pyref: pyref's 12 coefficients -> canonical tower coefficients"""
    vals = [0] * 12
    for j in range(2):
        for i in range(3):
            k = 2 * i + j
            c1 = p[k + 6]
            vals[2 * (3 * j + i)] = (p[k] + 9 * c1) % Q
            vals[2 * (3 * j + i) + 1] = c1
    return vals


def conj_words(vals):
    return vals[:6] + [(-v) % Q for v in vals[6:]]


def cyclotomic_cases(loose):
    rng = random.Random(1501)
    out = [("one", [ONE] + [0] * 11)]
    if loose:
        out.append(("loose one", [ONE + Q] + [Q] * 11))
    for i, g in enumerate(cyclotomic_values()):
        out.append(("g%d" % i, [mont(v) for v in g]))
        out.append(("conj g%d" % i, [mont(v) for v in conj_words(g)]))
        if loose:
            out.append(("g%d + q" % i, [mont(v) + Q for v in g]))
            out.append(("g%d mixed" % i, raw(g, rng, True)))
            out.append(("conj g%d mixed" % i, raw(conj_words(g), rng, True)))
    return out


def eq_cases(loose):
    """(label, a words + b words, expected flag): every pair of representatives of the same value, and near misses"""
    rng = random.Random(1601)
    out = []
    vals = [[0] * 12, [1] + [0] * 11, [rng.randrange(Q) for _ in range(12)], [Q - 1] * 12, [pow(RM, -1, Q)] * 12]
    for n, v in enumerate(vals):
        base = [mont(x) for x in v]
        reps = [base] + ([[x + Q for x in base], raw(v, rng, True), raw(v, rng, True)] if loose else [])
        for a in reps:
            for b in reps:
                out.append(("value %d, equal" % n, a + b, 1))
        for k in (0, 5, 11):                               # one coefficient different: by one limb's lowest bit, and by q - 1
            b = list(reps[-1]); b[k] = b[k] ^ 1
            out.append(("value %d, coefficient %d off by one" % (n, k), reps[0] + b, 0))
            b = list(reps[-1]); b[k] = (b[k] + (1 << 224)) % ((2 * Q) if loose else Q)
            out.append(("value %d, coefficient %d top limb off" % (n, k), reps[0] + b, 1 if b[k] % Q == reps[0][k] % Q else 0))
    return out


def is_one_cases(loose):
    out = [("one", [ONE] + [0] * 11, 1), ("zero", [0] * 12, 0), ("one + 1", [ONE + 1] + [0] * 11, 0), ("Montgomery 1 is not one", [1] + [0] * 11, 0)]
    for k in range(1, 12):
        w = [ONE] + [0] * 11; w[k] = 1
        out.append(("one, coefficient %d = 1 ulp" % k, w, 0))
    if loose:
        out += [("loose one", [ONE + Q] + [Q] * 11, 1), ("one with loose zeros", [ONE] + [Q] * 11, 1), ("loose one, c0.c0.c1 = q + 1", [ONE + Q, Q + 1] + [Q] * 10, 0),
                ("all q", [Q] * 12, 0), ("q + one only in the last", [Q] * 11 + [ONE + Q], 0)]
        for k in range(1, 12):
            w = [ONE + Q] + [0] * 11; w[k] = Q
            out.append(("loose one, coefficient %d = q" % k, w, 1))
    return out


def final_exp_cases(loose):
    """[(label, words, kind)]: kind "value" is compared with the reference, "one" / "zero" say what the reference gives without it"""
    rng = random.Random(1701)
    out = [("random 0", rand_words(rng, 12, loose), "value"), ("random 1", rand_words(rng, 12, loose), "value"),
           ("one", [ONE] + [0] * 11, "one"), ("in Fq6", rand_words(rng, 6, loose) + [0] * 6, "one"), ("zero", [0] * 12, "zero")]
    if loose:
        out += [("loose one", [ONE + Q] + [Q] * 11, "one"), ("in Fq6, loose zeros", rand_words(rng, 6, True) + [Q] * 6, "one"), ("loose zero", [Q] * 12, "zero")]
    return out


# ---------------------------------------------------------------- points
G1_SCALARS = [1, 2, R - 1, 0x1f2e3d4c5b6a79880796a5b4c3d2e1f00112233445566778899aabbccddeeff % R]
G2_SCALARS = [1, 2, R - 1, 0x2b5a1d3f9c7e6b8a4d2f1e0c9b8a7d6e5f4c3b2a19081726354453627180f % R]


@functools.lru_cache(maxsize=None)
def g1_point(k):
    return pyref.g1_mul(pyref.G1_GEN, k)


@functools.lru_cache(maxsize=None)
def g2_point(k):
    return pyref.g2_mul(pyref.G2_GEN, k)


def g1_words(P, rng=None, loose=False):
    if P is None:
        return [0, 0] if not (loose and rng and rng.getrandbits(1)) else [Q, Q]
    return raw([P[0], P[1]], rng, loose and rng is not None)


def g2_words(P, rng=None, loose=False):
    if P is None:
        return [0] * 4 if not (loose and rng and rng.getrandbits(1)) else [Q] * 4
    return raw([P[0][0], P[0][1], P[1][0], P[1][1]], rng, loose and rng is not None)


def hom_words(P, lam, rng, loose):
    """the twist point P as (lam X, lam Y, lam), lam in Fq2"""
    x, y = pyref.f2_mul(P[0], lam), pyref.f2_mul(P[1], lam)
    return raw([x[0], x[1], y[0], y[1], lam[0], lam[1]], rng, loose)


MEANINGLESS = ("Z = 0", "Z = loose 0")                       # pairing.hpp: T at infinity has no defined step; the domain invariant is all that is checked


def step_cases(add, loose):
    """[(label, words, m)]: T = [m]G2 scaled by a random lam; add: Q = G2 follows.  m = None marks the MEANINGLESS inputs"""
    rng = random.Random(1801 + add)
    out = []
    G2 = pyref.G2_GEN
    for m in (1, 2, 3, 5, R - 2, R - 3, G2_SCALARS[3]):
        if add and m == 1:
            continue
        for _ in range(2):
            lam = (rng.randrange(1, Q), rng.randrange(Q))
            out.append(("T = [%s]G2" % (m if m < 100 else hex(m)[:10]), hom_words(g2_point(m), lam, rng, loose) + (g2_words(G2, rng, loose) if add else []), m))
        out.append(("T = [%s]G2, Z = 1" % (m if m < 100 else hex(m)[:10]), hom_words(g2_point(m), (1, 0), None, False) + (g2_words(G2) if add else []), m))
    tail = g2_words(G2) if add else []
    out.append((MEANINGLESS[0], rand_words(rng, 4, loose) + [0, 0] + tail, None))
    if loose:
        out.append((MEANINGLESS[1], rand_words(rng, 4, loose) + [Q, Q] + tail, None))
    return out


def exceptional_add_cases(loose):
    """[(label, words, b_is_zero)]: T = Q (the addition degenerates: Z', a, b all vanish) and T = -Q (Z', a vanish, b does not)"""
    rng = random.Random(1901)
    out = []
    for k in (1, 2, G2_SCALARS[3]):
        P = g2_point(k)
        nP = (P[0], pyref.f2_neg(P[1]))
        for _ in range(2):
            lam = (rng.randrange(1, Q), rng.randrange(Q))
            out.append(("T = Q", hom_words(P, lam, rng, loose) + g2_words(P, rng, loose), True))
            out.append(("T = -Q", hom_words(nP, lam, rng, loose) + g2_words(P, rng, loose), False))
        out.append(("T = Q, Z = 1", hom_words(P, (1, 0), None, False) + g2_words(P), True))
    return out


def ell_cases(loose):
    """[(label, words, skip)]"""
    rng = random.Random(2001)
    out = []
    for i, (la, f) in enumerate(elements(12, loose, 2000, n_drawn=4, n_random=4)):
        line = rand_words(rng, 6, loose)
        if i % 4 == 0:
            line[2 * (i % 3):2 * (i % 3) + 2] = [Q if loose else 0, 0]
        P = g1_words(g1_point(G1_SCALARS[i % 4]), rng, loose)
        for skip in (0, 1):
            out.append(("%s skip %d" % (la, skip), f + line + P + [skip], skip))
    return out


MILLER_PAIRS = [(1, 1), (2, R - 1), (R - 1, 2), (G1_SCALARS[3], G2_SCALARS[3]), (1, G2_SCALARS[3]), (G1_SCALARS[3], 1)]


def pair_words(pairs, rng, loose):
    """operands of the miller / pair_product ops: the G1 points, then the G2 points ((a, b) scalars; None = infinity)"""
    w = []
    for a, _ in pairs:
        w += g1_words(None if a is None else g1_point(a), rng, loose)
    for _, b in pairs:
        w += g2_words(None if b is None else g2_point(b), rng, loose)
    return w


def twist_points():
    """[(label, point or None, on_curve, in_subgroup)]"""
    G2 = pyref.G2_GEN
    out = [("O", None, True, True), ("G2", G2, True, True), ("-G2", (G2[0], pyref.f2_neg(G2[1])), True, True)]
    out += [("[%s]G2" % n, g2_point(k), True, True) for n, k in (("2", 2), ("r-1", R - 1), ("(r+1)/2", (R + 1) // 2))]
    cof = 2 * Q - R
    assert cof % 10069 == 0
    base = V.twist_point_outside_subgroup(11)
    low = V.g2_mul_raw(base, cof * R // 10069)
    assert low is not None and V.g2_mul_raw(low, 10069) is None
    out.append(("order 10069", low, True, False))
    out.append(("order 10069 r", pyref.g2_add(G2, low), True, False))
    out += [("random twist point %d" % s, V.twist_point_outside_subgroup(s), True, False) for s in (12, 13)]
    out.append(("G2 with y + 1", (G2[0], pyref.f2_add(G2[1], (1, 0))), False, None))
    out.append(("G2 with x.c1 + 1", (pyref.f2_add(G2[0], (0, 1)), G2[1]), False, None))
    out.append(("(0, 1)", ((0, 0), (1, 0)), False, None))
    return out


# ---------------------------------------------------------------- the prepare kernel
BLIND_C, BLIND_D, BLIND_W = 6, 32, 43
PREP_K = [0x1d3f9c7e6b8a4d2f1e0c9b8a7d6e5f4c3b2a19081726354453627180f0e1d2c % R, 0x7e6b8a4d2f1e0c9b8a7d6e5f4c3b2a1908172635445362 % R, 5]


def digits_scalar(d, top):
    """the scalar whose base-2^BLIND_C digits are d in the windows 0 .. BLIND_W - 2 and `top` in the last (which holds two bits)"""
    return sum(d << (BLIND_C * w) for w in range(BLIND_W - 1)) + (top << (BLIND_C * (BLIND_W - 1)))


def prepare_inputs():
    """[(label, (s1, s2))] for the key gammaABC = [k0 G1, k1 G1, k2 G1]"""
    k0, k1, k2 = PREP_K
    inv = lambda v: pow(v, -1, R)
    s_inf1 = (-k0) * inv(k1) % R                           # k0 + s1 k1 = 0: the accumulator is infinity after the first term
    out = [("0, 0", (0, 0)), ("1, 1", (1, 1)), ("r - 1, r - 1", (R - 1, R - 1)), ("0, r - 1", (0, R - 1)), ("r - 1, 0", (R - 1, 0)),
           ("digits all BLIND_D", (digits_scalar(BLIND_D, 1), digits_scalar(BLIND_D, 2))),
           ("digits all BLIND_D + 1", (digits_scalar(BLIND_D + 1, 1), digits_scalar(BLIND_D + 1, 0))),
           ("digits all 2^BLIND_C - 1", (digits_scalar(63, 1), digits_scalar(63, 2))),
           ("digits BLIND_D - 1 / BLIND_D alternating", (sum((BLIND_D - (w & 1)) << (6 * w) for w in range(42)), 7)),
           ("accumulator infinite after the first term", (s_inf1, 12345)),
           ("accumulator infinite after the first term, s2 = 0", (s_inf1, 0)),
           ("final sum infinite", (3, (-(k0 + 3 * k1)) * inv(k2) % R)),
           ("second term equals the accumulator", (3, (k0 + 3 * k1) * inv(k2) % R)),
           ("second term equals the accumulator, s1 = 0", (0, k0 * inv(k2) % R)),
           ("first term equals gammaABC[0]", (k0 * inv(k1) % R, 9)),
           ("random", (0x2b5a1d3f9c7e6b8a4d2f1e0c9b8a7d6e5f4c3b2a19081726354453627180f % R, 0x1234567890abcdef))]
    return out


def prepare_expected_scalar(s, k=PREP_K):
    return (k[0] + sum(si * ki for si, ki in zip(s, k[1:]))) % R


# ---------------------------------------------------------------- premises
def premises():
    """from the reference alone: the lists hold the kinds the issue names"""
    for width in (2, 6, 12):
        coeffs = {w for _, ws in elements(width, True, 1) for w in ws}
        assert set(edge_values(True)) <= coeffs
        labels = [l for l, _ in elements(width, True, 1)]
        assert "loose one" in labels
        assert any(ws == [2 * Q - 1] * width for _, ws in elements(width, True, 1)) and any(ws == [Q] * width for _, ws in elements(width, True, 1))
        assert all(w < 2 * Q for w in coeffs) and all(w < Q for _, ws in elements(width, False, 1) for w in ws)
    for loose in (False, True):
        # Karatsuba sums that vanish, in both representatives of zero when loose
        sums = {(a[k] + a[6 + k]) for _, ws in f12_pairs(loose) for a in (ws[:12],) for k in range(6) if (a[k] + a[6 + k]) % Q == 0 and a[k] % Q}
        assert (sums >= {Q, 2 * Q}) if loose else (sums == {Q})
        sums6 = {(ws[k] + ws[j + k]) for _, ws in f6_pairs(loose) for j in (2, 4) for k in range(2) if (ws[k] + ws[j + k]) % Q == 0 and ws[k] % Q}
        assert (sums6 >= {Q, 2 * Q}) if loose else (sums6 == {Q})
        assert any(all(w % Q == 0 for w in ws[6:12]) and any(w % Q for w in ws[:6]) for _, ws in f12_pairs(loose))
        assert any(l.startswith("b sparse") for l, _ in f12_pairs(loose))
        assert any(any(ws[12 + 2 * k] % Q == 0 and ws[13 + 2 * k] % Q == 0 for k in range(3)) for _, ws in mul034_cases(loose))
        # inversions: zero in every representative, two zero coefficients
        zeros = [ws for _, ws in f12_unary(loose) if all(w % Q == 0 for w in ws)]
        assert [0] * 12 in zeros and (not loose or [Q] * 12 in zeros)
        assert sum(1 for _, ws in f6_unary(loose) if sum(1 for k in range(3) if ws[2 * k] % Q == 0 and ws[2 * k + 1] % Q == 0) == 2) >= 9
        # predicates: both answers, near misses
        assert {f for _, _, f in eq_cases(loose)} == {0, 1} and {f for _, _, f in is_one_cases(loose)} == {0, 1}
        for _, ws, f in eq_cases(loose):
            assert f == int(all((a - b) % Q == 0 for a, b in zip(ws[:12], ws[12:])))
        for _, ws, f in is_one_cases(loose):
            assert f == int(ws[0] % Q == ONE and all(w % Q == 0 for w in ws[1:]))
        if loose:
            assert any(f and ws[:12] != ws[12:] for _, ws, f in eq_cases(True))
        assert sum(1 for l, _ in frob_cases(loose) if l.startswith("basis")) == 12
        assert {k for _, _, k in final_exp_cases(loose)} == {"value", "one", "zero"}
        # steps: scaled points, the meaningless inputs are exactly the named ones
        for add in (0, 1):
            cs = step_cases(add, loose)
            assert [l for l, _, m in cs if m is None] == list(MEANINGLESS[:2 if loose else 1])
            assert all((ws[4] % Q, ws[5] % Q) != (0, 0) for _, ws, m in cs if m is not None)
            assert any((dm(ws[4]), dm(ws[5])) != (1, 0) for _, ws, m in cs if m is not None)
        assert {b for _, _, b in exceptional_add_cases(loose)} == {True, False}
        assert {s for _, _, s in ell_cases(loose)} == {0, 1}
    assert {a for a, _ in MILLER_PAIRS} >= {1, 2, R - 1} and {b for _, b in MILLER_PAIRS} >= {1, 2, R - 1}
    kinds = {(c, s) for _, _, c, s in twist_points()}
    assert kinds == {(True, True), (True, False), (False, None)}
    for _, P, c, s in twist_points():
        assert pyref.g2_on_curve(P) == c
        if c:
            assert (V.g2_mul_raw(P, R) is None) == s if P is not None else s
    # the prepare kernel's scalars
    k0, k1, k2 = PREP_K
    dig = lambda s: [(s >> (6 * w)) & 63 for w in range(BLIND_W)]
    ins = dict(prepare_inputs())
    assert all(0 <= s < R for pair in ins.values() for s in pair)
    assert set(dig(ins["digits all BLIND_D"][0])[:42]) == {BLIND_D} and set(dig(ins["digits all BLIND_D + 1"][0])[:42]) == {BLIND_D + 1}
    assert set(dig(ins["digits all 2^BLIND_C - 1"][0])[:42]) == {63}
    s = ins["accumulator infinite after the first term"]
    assert (k0 + s[0] * k1) % R == 0 and prepare_expected_scalar(s) != 0
    assert prepare_expected_scalar(ins["final sum infinite"]) == 0
    s = ins["second term equals the accumulator"]
    assert (k0 + s[0] * k1) % R == s[1] * k2 % R != 0
