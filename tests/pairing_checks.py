"""What the pairing-probe tests assert, shared by test_pairing_emul.py and test_pairing_gpu.py: every check takes the binding (`zk`, the
emulation verifier library or the device library loaded into ethsnarks_amd.prover) and compares zk.pairing_probe with oracle/pyref.py
(Python integers; tower elements through verify_batch_cases.tower_to_pyref) over the lists of tests/pairing_cases.py.

Two assertions per case and output coefficient: the VALUE is congruent to the reference modulo q -- exactly, there is no tolerance -- and
the raw word lies in the DOMAIN [0, 2q) ([0, q) where the function is documented strict).  Projective points and lines are compared by
cross-multiplication: the device scales them by Fq2 factors.  No case is skipped or filtered; the one input pairing.hpp declares
meaningless (a step from T with Z = 0) is checked for the domain invariant only.  One launch per op and operand list."""
import functools

import numpy as np
import pyref
from ethsnarks_amd import fields as F
import pairing_cases as K
import verify_batch_cases as V

Q, R = K.Q, K.R
MAX_SHOWN = 4
F12_ZERO = [0] * 12


def _hx(ws):
    return "[" + ", ".join("%#x" % w for w in ws) + "]"


def _report(what, failures):
    assert not failures, "%s: %d case(s) fail, the first:\n  " % (what, len(failures)) + "\n  ".join(failures[:MAX_SHOWN])


def run(zk, name, cases):
    """cases: list of operand word lists -> list of result word lists (raw integers); checks the shape the header documents"""
    wi, wo = K.SHAPES[name]
    assert zk.pairing_probe_shape(K.OPS[name]) == (wi, wo), name
    assert all(len(c) == wi for c in cases), name
    out = zk.pairing_probe(K.OPS[name], F.ints_to_limbs([w for c in cases for w in c]).reshape(len(cases), wi, 4))
    flat = F.limbs_to_ints(out)
    return [flat[i * wo:(i + 1) * wo] for i in range(len(cases))]


def domain_errors(name, words):
    bound = Q if name in K.STRICT_RESULT else 2 * Q
    return ["word %d = %#x is not below %s" % (i, w, "q" if bound == Q else "2q") for i, w in enumerate(words) if w >= bound]


# ---- raw words -> reference values
def t2(ws):
    return (K.dm(ws[0]), K.dm(ws[1]))


def t12(ws):
    return V.tower_to_pyref([K.dm(w) for w in ws])


def t6(ws):
    return t12(list(ws) + [0] * 6)


def e2(a):
    return pyref._embed([(0, a)])


V_ELEM = [0, 0, 1] + [0] * 9                              # v = w^2


def line_element(l, P):
    """the sparse element a y_P + (b x_P) w + c v w of pairing.hpp"""
    return pyref._embed([(0, pyref.f2_muls(l[0], P[1])), (1, pyref.f2_muls(l[1], P[0])), (3, l[2])])


def conj12(p):
    return [(-c) % Q if i & 1 else c for i, c in enumerate(p)]         # w -> -w


def check_values(zk, name, cases, expect, what=None):
    """cases: [(label, words, ...)]; expect(case, got words) -> list of error strings"""
    got = run(zk, name, [c[1] for c in cases])
    bad = []
    for i, (c, g) in enumerate(zip(cases, got)):
        errs = domain_errors(name, g) + expect(c, g)
        if errs:
            bad.append("%s case %d (%s) operands %s: got %s: %s" % (name, i, c[0], _hx(c[1]), _hx(g), "; ".join(errs)))
    _report("%s (%d cases)" % (what or name, len(cases)), bad)
    return got


def _eq(got_ref, want_ref, what="value"):
    return [] if got_ref == want_ref else ["%s differs from the reference (mod q): want %s" % (what, _hx(want_ref))]


# ---------------------------------------------------------------- Fq2 helpers and Fq6
def check_fq2_helpers(zk, loose):
    el = K.elements(2, loose, 20, n_drawn=12, n_random=8)
    check_values(zk, "f2mulxi", el, lambda c, g: _eq(list(t2(g)), list(pyref.f2_mul(t2(c[1]), pyref.XI))))
    check_values(zk, "f2conj", el, lambda c, g: _eq(list(t2(g)), list(pyref.f2_conj(t2(c[1])))))
    ev = K.edge_values(loose)
    cases = [(l + " s = %#x.." % (s >> 224), ws + [s]) for l, ws in el for s in ev[:3] + ev[-2:]]
    check_values(zk, "f2muls", cases, lambda c, g: _eq(list(t2(g)), list(pyref.f2_muls(t2(c[1]), K.dm(c[1][2])))))


def check_fq6(zk, loose):
    pairs = K.f6_pairs(loose)
    mul = lambda c, g: _eq(t6(g), pyref.f12_mul(t6(c[1][:6]), t6(c[1][6:])))
    plain = check_values(zk, "f6mul", pairs, mul)
    alias = check_values(zk, "f6mul_alias", pairs, mul)
    _report("f6mul with the output aliasing the first operand", ["case %d (%s)" % (i, pairs[i][0]) for i in range(len(pairs)) if [w % Q for w in plain[i]] != [w % Q for w in alias[i]]])
    coeff = lambda op: (lambda c, g: _eq([K.dm(w) for w in g], [op(K.dm(a), K.dm(b)) % Q for a, b in zip(c[1][:6], c[1][6:])]))
    check_values(zk, "f6add", pairs, coeff(lambda a, b: a + b))
    check_values(zk, "f6sub", pairs, coeff(lambda a, b: a - b))
    un = K.f6_unary(loose)
    check_values(zk, "f6neg", un, lambda c, g: _eq([K.dm(w) for w in g], [(-K.dm(a)) % Q for a in c[1]]))
    check_values(zk, "f6mulv", un, lambda c, g: _eq(t6(g), pyref.f12_mul(t6(c[1]), V_ELEM)))
    def inv(c, g):
        a = t6(c[1])
        return _eq(t6(g), F12_ZERO, "1/0") if a == F12_ZERO else _eq(pyref.f12_mul(a, t6(g)), pyref.F12_ONE, "a * result")
    check_values(zk, "f6inv", un, inv)
    m01 = [(l, ws[:10]) for l, ws in pairs]
    check_values(zk, "f6mul01", m01, lambda c, g: _eq(t6(g), pyref.f12_mul(t6(c[1][:6]), t6(c[1][6:10] + [0, 0]))))


# ---------------------------------------------------------------- Fq12
def _same_mod_q(what, cases, a, b):
    _report(what, ["case %d (%s): %s against %s" % (i, cases[i][0], _hx(a[i]), _hx(b[i])) for i in range(len(cases)) if [w % Q for w in a[i]] != [w % Q for w in b[i]]])


def check_f12_mul(zk, loose):
    pairs = K.f12_pairs(loose)
    mul = lambda c, g: _eq(t12(g), pyref.f12_mul(t12(c[1][:12]), t12(c[1][12:])))
    plain = check_values(zk, "f12mul", pairs, mul)
    alias = check_values(zk, "f12mul_alias", pairs, mul)
    _same_mod_q("f12mul with the output aliasing the first operand", pairs, plain, alias)
    # the sparse operands through f12mul034: the same values as the dense product
    sp = [(l, ws[:12] + ws[12:14] + ws[18:22]) for l, ws in pairs if l.startswith("b sparse")]
    dense = [plain[i] for i, (l, _) in enumerate(pairs) if l.startswith("b sparse")]
    assert sp
    got = run(zk, "f12mul034", [c[1] for c in sp])
    _same_mod_q("f12mul034 against the dense f12mul", sp, got, dense)


def check_f12_mul034(zk, loose):
    cases = K.mul034_cases(loose)
    check_values(zk, "f12mul034", cases, lambda c, g: _eq(t12(g), pyref.f12_mul(t12(c[1][:12]), t12(K.sparse034(c[1][12:18])))))


def check_f12_sqr_conj_canon(zk, loose):
    un = K.f12_unary(loose)
    sq = lambda c, g: _eq(t12(g), pyref.f12_mul(t12(c[1]), t12(c[1])))
    plain = check_values(zk, "f12sqr", un, sq)
    alias = check_values(zk, "f12sqr_alias", un, sq)
    _same_mod_q("f12sqr with the output aliasing the input", un, plain, alias)
    a = t12(un[-1][1])
    assert conj12(a) == pyref.f12_pow(a, Q ** 6)                                       # the reference's conjugation is the q^6 map
    check_values(zk, "f12conj", un, lambda c, g: _eq(t12(g), conj12(t12(c[1]))))
    check_values(zk, "f12canon", un, lambda c, g: [] if g == [w % Q for w in c[1]] else ["not the input reduced into [0, q)"])


def check_f12_inv(zk, loose):
    un = K.f12_unary(loose)
    def inv(c, g):
        a = t12(c[1])
        return _eq(t12(g), F12_ZERO, "1/0") if a == F12_ZERO else _eq(pyref.f12_mul(a, t12(g)), pyref.F12_ONE, "a * result")
    plain = check_values(zk, "f12inv", un, inv)
    alias = check_values(zk, "f12inv_alias", un, inv)
    _same_mod_q("f12inv with the output aliasing the input", un, plain, alias)


def check_f12_frobenius(zk, loose, k):
    cases = K.frob_cases(loose)
    check_values(zk, "f12frob%d" % k, cases, lambda c, g: _eq(t12(g), pyref.f12_pow(t12(c[1]), Q ** k)))


def check_f12_predicates(zk, loose):
    check_values(zk, "f12eq", K.eq_cases(loose), lambda c, g: [] if g == [c[2]] else ["want %d" % c[2]])
    check_values(zk, "f12is_one", K.is_one_cases(loose), lambda c, g: [] if g == [c[2]] else ["want %d" % c[2]])


def check_cyclotomic(zk, loose):
    cases = K.cyclotomic_cases(loose)
    sq = lambda c, g: _eq(t12(g), pyref.f12_mul(t12(c[1]), t12(c[1])))
    plain = check_values(zk, "f12cycsqr", cases, sq)
    alias = check_values(zk, "f12cycsqr_alias", cases, sq)
    _same_mod_q("f12cycsqr with the output aliasing the input", cases, plain, alias)
    _same_mod_q("f12cycsqr against f12sqr in the cyclotomic subgroup", cases, plain, run(zk, "f12sqr", [c[1] for c in cases]))
    check_values(zk, "f12exp_negz", cases, lambda c, g: _eq(t12(g), conj12(pyref.f12_pow(t12(c[1]), V.BN_Z))))


@functools.lru_cache(maxsize=None)
def _ref_easy(key):
    return pyref.f12_pow(list(key), K.EASY_POWER)


@functools.lru_cache(maxsize=None)
def _ref_final(key):
    return pyref.f12_pow(pyref.final_exp(list(key)), V.FE_CHAIN_POWER)


def check_final_exp(zk, loose):
    cases = K.final_exp_cases(loose)
    def expect(fn):
        def e(c, g):
            a = t12(c[1])
            if c[2] == "zero":
                assert a == F12_ZERO
                return _eq(t12(g), F12_ZERO, "f(0)")
            want = fn(tuple(a))
            if c[2] == "one" and fn is _ref_final:
                assert want == pyref.F12_ONE                                          # (q^6 - 1 kills Fq6)
            return _eq(t12(g), want)
        return e
    check_values(zk, "final_exp_easy", cases, expect(_ref_easy))
    check_values(zk, "final_exp", cases, expect(_ref_final))


# ---------------------------------------------------------------- the Miller steps
def _unembed(l, k):
    return ((l[k] + 9 * l[k + 6]) % Q, l[k + 6])


def ref_line(T, Qp):
    """(1, -lambda, lambda x_T - y_T) of the line through T and Qp (the tangent for T = Qp) and T + Qp, from pyref._line"""
    l, S = pyref._line(T, Qp, (1, 1))
    return (_unembed(l, 0), _unembed(l, 1), _unembed(l, 3)), S


def _step_errors(g, want_pt, want_line):
    m = pyref.f2_mul
    X, Y, Z, a, b, c = [t2(g[2 * i:2 * i + 2]) for i in range(6)]
    errs = []
    if Z == (0, 0):
        errs.append("Z' = 0")
    if X != m(want_pt[0], Z) or Y != m(want_pt[1], Z):
        errs.append("T' is not projectively the reference point")
    ra, rb, rc = want_line
    assert ra == (1, 0)
    if a == (0, 0) or b != m(a, rb) or c != m(a, rc):
        errs.append("the line is not proportional to the reference line")
    return errs


def check_steps(zk, loose):
    G2 = pyref.G2_GEN
    def expect(add):
        def e(c, g):
            if c[2] is None:
                assert c[0] in K.MEANINGLESS
                return []                                                              # domain only (check_values has done it)
            T = K.g2_point(c[2])
            line, S = ref_line(T, G2 if add else T)
            assert S == K.g2_point(c[2] + 1 if add else 2 * c[2])
            return _step_errors(g, S, line)
        return e
    check_values(zk, "dbl_step", K.step_cases(0, loose), expect(0))
    check_values(zk, "add_step", K.step_cases(1, loose), expect(1))
    def exceptional(c, g):
        Z, a, b = t2(g[4:6]), t2(g[6:8]), t2(g[8:10])
        errs = []
        if Z != (0, 0): errs.append("Z' != 0")
        if a != (0, 0): errs.append("l.a != 0")
        if (b == (0, 0)) != c[2]: errs.append("l.b is %szero" % ("" if b == (0, 0) else "not "))
        return errs
    check_values(zk, "add_step", K.exceptional_add_cases(loose), exceptional, "add_step at T = +-Q")


def check_g2_frobenius(zk, loose):
    import random
    rng = random.Random(2101)
    cases = [("[%#x..]G2" % (k & 0xffff), K.g2_words(K.g2_point(k), rng, loose)) for k in K.G2_SCALARS for _ in range(2)]
    g12, g13 = pyref.f2_pow(pyref.XI, (Q - 1) // 3), pyref.f2_pow(pyref.XI, (Q - 1) // 2)
    g22 = pyref.f2_pow(pyref.XI, (Q * Q - 1) // 3)
    pt = lambda ws: (t2(ws[0:2]), t2(ws[2:4]))
    check_values(zk, "g2_frob1", cases, lambda c, g: [] if pt(g) == (pyref.f2_mul(pyref.f2_conj(pt(c[1])[0]), g12), pyref.f2_mul(pyref.f2_conj(pt(c[1])[1]), g13)) else ["not pi(Q)"])
    check_values(zk, "g2_negfrob2", cases, lambda c, g: [] if pt(g) == (pyref.f2_mul(pt(c[1])[0], g22), pt(c[1])[1]) else ["not -pi^2(Q)"])


def check_ell(zk, loose):
    def expect(c, g):
        ws = c[1]
        f = t12(ws[:12])
        if c[2]:
            return _eq(t12(g), f, "f (skip = 1 leaves it unchanged)")
        l = [t2(ws[12 + 2 * i:14 + 2 * i]) for i in range(3)]
        return _eq(t12(g), pyref.f12_mul(f, line_element(l, (K.dm(ws[18]), K.dm(ws[19])))))
    check_values(zk, "ell", K.ell_cases(loose), expect)


# ---------------------------------------------------------------- the Miller loop
@functools.lru_cache(maxsize=None)
def _ref_miller_easy(a, b):
    return pyref.f12_pow(pyref.miller_loop(K.g2_point(b), K.g1_point(a)), K.EASY_POWER)


def check_miller(zk, loose):
    """variable-Q singles against the reference (after the easy part, which removes the Fq2 scalings of the lines); nv = 2, 3 and the
    fixed-Q route against products of the device's own singles, exactly; infinity and fskip contribute exactly 1"""
    import random
    rng = random.Random(2201)
    singles = list(K.MILLER_PAIRS) + [(None, 1), (1, None), (None, None)]
    cases = [("P = %s, Q = %s" % (a if a is None or a < 100 else "a", b if b is None or b < 100 else "b"), K.pair_words([(a, b)], rng, loose), (a, b)) for a, b in singles]
    def expect(c, g):
        a, b = c[2]
        if a is None or b is None:
            return _eq(t12(g), pyref.F12_ONE, "f for a pair with infinity")
        return _eq(_ref_easy(tuple(t12(g))), _ref_miller_easy(a, b), "f^((q^6-1)(q^2+1))")
    got = check_values(zk, "miller1", cases, expect)
    f = {c[2]: t12(g) for c, g in zip(cases, got)}
    prod = lambda pairs: functools.reduce(pyref.f12_mul, [f[p] for p in pairs], pyref.F12_ONE)
    P = K.MILLER_PAIRS
    m2 = [[P[0], P[1]], [P[3], P[2]], [(None, 1), P[4]], [P[5], (1, None)], [(None, None), (None, 1)], [P[2], P[2]]]
    m3 = [[P[0], P[1], P[2]], [P[3], (None, 1), P[4]], [(1, None), P[5], P[0]], [P[1], P[3], (None, None)]]
    for name, groups in (("miller2", m2), ("miller3", m3)):
        cs = [("pairs %d" % i, K.pair_words(g, rng, loose), g) for i, g in enumerate(groups)]
        check_values(zk, name, cs, lambda c, g: _eq(t12(g), prod(c[2]), "f against the product of the single-pair values"))
    # fixed-Q route: the same value as the variable-Q walk of the same pair; fskip or P at infinity give 1
    fx1 = [("pair %d, fskip %d" % (i, s), K.pair_words([p], rng, loose) + [s], [] if s & 1 else [p]) for i, p in enumerate(P) for s in ((0, 1) if i < 2 else (0,))]
    fx1 += [("P at infinity", K.pair_words([(None, 2)], rng, loose) + [0], []), ("fskip bit 1 is not this pair's", K.pair_words([P[1]], rng, loose) + [2], [P[1]])]
    check_values(zk, "miller_fixed1", fx1, lambda c, g: _eq(t12(g), prod(c[2]), "f against the variable-Q value"))
    fx2 = []
    for i, (p0, p1) in enumerate([(P[0], P[1]), (P[3], P[2]), (P[4], P[5])]):
        for s in (0, 1, 2, 3) if i == 0 else (0, 1 + (i & 1)):
            fx2.append(("pairs %d, fskip %d" % (i, s), K.pair_words([p0, p1], rng, loose) + [s], [p for j, p in enumerate((p0, p1)) if not (s >> j) & 1]))
    fx2.append(("first P at infinity", K.pair_words([(None, 2), P[1]], rng, loose) + [0], [P[1]]))
    fx2.append(("second P at infinity", K.pair_words([P[3], (None, R - 1)], rng, loose) + [0], [P[3]]))
    check_values(zk, "miller_fixed2", fx2, lambda c, g: _eq(t12(g), prod(c[2]), "f against the variable-Q values"))


@functools.lru_cache(maxsize=None)
def _ref_pairing(a, b):
    return _ref_final(tuple(pyref.miller_loop(K.g2_point(b), K.g1_point(a))))


def check_pair_product(zk, loose):
    """k_pair_product's values: 67 cases in one launch (a second block, a ragged wave) over three distinct pairings and infinity, every
    position against the reference; n = 2, 3 against products of the reference values (the exponentiation is multiplicative)"""
    import random
    rng = random.Random(2301)
    distinct = [K.MILLER_PAIRS[0], K.MILLER_PAIRS[1], K.MILLER_PAIRS[3], (None, 1)]
    ref = lambda p: pyref.F12_ONE if p[0] is None or p[1] is None else _ref_pairing(*p)
    cases = [("lane %d" % i, K.pair_words([distinct[(i * 3 + i // 64) % 4]], rng, loose), [distinct[(i * 3 + i // 64) % 4]]) for i in range(67)]
    assert len({tuple(c[2]) for c in (cases[0], cases[63], cases[64], cases[66])}) >= 3
    prod = lambda c, g: _eq(t12(g), functools.reduce(pyref.f12_mul, [ref(p) for p in c[2]], pyref.F12_ONE))
    check_values(zk, "pair_product1", cases, prod)
    d = distinct
    c2 = [("pairs %d" % i, K.pair_words(g, rng, loose), g) for i, g in enumerate([[d[0], d[1]], [d[2], d[3]], [d[1], d[1]]])]
    check_values(zk, "pair_product2", c2, prod)
    c3 = [("pairs %d" % i, K.pair_words(g, rng, loose), g) for i, g in enumerate([[d[0], d[1], d[2]], [d[3], d[2], d[0]]])]
    check_values(zk, "pair_product3", c3, prod)


# ---------------------------------------------------------------- predicates
def check_point_predicates(zk, loose):
    import random
    rng = random.Random(2401)
    pts = K.twist_points()
    reps = [None] + ([rng, rng] if loose else [])
    on = [(l, K.g2_words(P, r, loose), int(c)) for l, P, c, _ in pts for r in reps]
    if loose:
        on.append(("O as (q, q, q, q)", [Q] * 4, 1))
    check_values(zk, "g2_on_curve", on, lambda c, g: [] if g == [c[2]] else ["want %d" % c[2]])
    sub = [(l, K.g2_words(P, r, loose), int(s)) for l, P, c, s in pts if c for r in reps]
    check_values(zk, "g2_in_subgroup", sub, lambda c, g: [] if g == [c[2]] else ["want %d" % c[2]])
    g1 = [("[%#x..]G1" % (k & 0xffff), K.g1_point(k), 1) for k in K.G1_SCALARS] + [("O", None, 1), ("(1, 3)", (1, 3), 0), ("(0, 1)", (0, 1), 0), ("(2, 2)", (2, 2), 0)]
    g1 += [("G1 with x + 1", (2, 2), 0), ("-G1", (1, Q - 2), 1)]
    cs = [(l, K.g1_words(P, r, loose), f) for l, P, f in g1 for r in reps]
    for _, ws, f in cs:
        x, y = K.dm(ws[0]), K.dm(ws[1])
        assert f == int((x, y) == (0, 0) or (y * y - x ** 3 - 3) % Q == 0)
    check_values(zk, "g1_on_curve", cs, lambda c, g: [] if g == [c[2]] else ["want %d" % c[2]])


# ---------------------------------------------------------------- the prepare kernel
def _vk_json(ks):
    import json
    G1, G2 = pyref.G1_GEN, pyref.G2_GEN
    vk = dict(alpha_g1=pyref.g1_mul(G1, 7), beta_g2=pyref.g2_mul(G2, 11), gamma_g2=pyref.g2_mul(G2, 13), delta_g2=pyref.g2_mul(G2, 17),
              gamma_abc=[pyref.g1_mul(G1, k) for k in ks])
    return json.dumps(pyref.vk_to_json_dict(vk))


def _record(zk, A, B, C):
    p = zk.ZkProof()
    for name, v in zip(("a_x", "a_y", "b_x_c0", "b_x_c1", "b_y_c0", "b_y_c1", "c_x", "c_y"), (A[0], A[1], B[0][0], B[0][1], B[1][0], B[1][1], C[0], C[1])):
        limbs = F.ints_to_limbs([v])[0]
        for j in range(4):
            getattr(p, name)[j] = int(limbs[j])
    return p


def check_prepare(zk, make_verifier):
    """k_vfy_prepare alone (zk_vctx_probe_prepare): nAcc = -(k0 + sum s_j k_j) G1 in affine, (0, 0) for the sum 0; A, nC, B as decoded;
    `ok`; every word below 2q.  make_verifier(vk_json, max_batch) -> zk.Verifier (the caller sets the table budget)"""
    G1, G2 = pyref.G1_GEN, pyref.G2_GEN
    A, B, Cp = pyref.g1_mul(G1, 21), pyref.g2_mul(G2, 22), pyref.g1_mul(G1, 23)
    good = K.prepare_inputs()
    bad = [("a coordinate equal to q", (Q, A[1]), Cp, (1, 2)), ("an input equal to r", A, Cp, (R, 2)), ("A off the curve", (A[0], (A[1] + 1) % Q), Cp, (1, 2)),
           ("C off the curve", A, ((Cp[0] + 1) % Q, Cp[1]), (1, 2)), ("second input 2^256 - 1", A, Cp, (1, (1 << 256) - 1))]
    rows = [(l, A, Cp, s, 1) for l, s in good] + [(l, a, c, s, 0) for l, a, c, s in bad]
    assert len(rows) >= 17
    for nIn, ks in ((2, K.PREP_K), (0, K.PREP_K[:1])):
        ver = make_verifier(_vk_json(ks), len(rows))
        for k in sorted({17, len(rows)}):                                              # 17: a block of 64 lanes holds 16 quads, the 17th is a ragged one
            use = rows[-k:] if k < len(rows) else rows
            recs = [_record(zk, a, B, c) for _, a, c, _, _ in use]
            inp = F.ints_to_limbs([v for _, _, _, s, _ in use for v in s[:nIn]]).reshape(len(use), nIn, 4) if nIn else np.zeros((len(use), 0, 4), dtype=np.uint64)
            pts, ok = ver.probe_prepare(recs, inp)
            bad_rows = []
            for i, ((label, a, c, s, want_ok), words) in enumerate(zip(use, [F.limbs_to_ints(pts[j]) for j in range(len(use))])):
                errs = ["word %d = %#x is not below 2q" % (j, w) for j, w in enumerate(words) if w >= 2 * Q]
                if nIn == 0:
                    want_ok = int(label not in ("a coordinate equal to q", "A off the curve", "C off the curve"))
                if ok[i] != want_ok:
                    errs.append("ok = %d, want %d" % (ok[i], want_ok))
                if want_ok:
                    v = [K.dm(w) for w in words]
                    e = K.prepare_expected_scalar(s[:nIn], ks)
                    acc = pyref.g1_neg(pyref.g1_mul(G1, e)) if e else None
                    if (v[2], v[3]) != ((0, 0) if acc is None else acc):
                        errs.append("nAcc is not -(%#x) G1" % e)
                    if (v[0], v[1]) != a: errs.append("A differs")
                    if (v[4], v[5]) != pyref.g1_neg(c): errs.append("nC is not -C")
                    if ((v[6], v[7]), (v[8], v[9])) != B: errs.append("B differs")
                if errs:
                    bad_rows.append("record %d (%s, nIn = %d, k = %d): %s: %s" % (i, label, nIn, k, _hx(words), "; ".join(errs)))
            _report("k_vfy_prepare (nIn = %d, k = %d)" % (nIn, k), bad_rows)
        ver.close()
