"""Operand lists and checks for the dedicated field squaring (csrc/bn254.hpp, Field::lsqr / lsqr_pair: sqr_fips, sqr_fips_x2 on the device,
sqr_cols_c in plain C++), shared by test_fq_squaring_emul.py and test_fq_squaring_gpu.py.  Both run the SAME operand list through the
arithmetic probe (field ops 6 lmul, 7 lsqr, 26 lsqr_pair).

Field list (raw limb values of the loose domain [0, 2p)): 0, 1, p - 1, p, p + 1, 2p - 1, R mod p, all-ones limbs masked below 2p
(2^254 - 1), one limb of ones at each of the eight positions (the top one masked below 2p), alternating 0 / 0xffffffff limbs in both phases
(the largest column sums: every product of a column is (2^32 - 1)^2 or 0, and the doubled limbs are all ones), and 256 seeded random values
of [0, 2p).
Contract: lsqr(a) = a^2 R^-1 (mod p) and below 2p; its canonical form is that of lmul(a, a); and, stronger, the RAW limbs equal lmul(a, a)'s:
both forms sum the same integer a^2 into the columns, the Montgomery multiplier m = -a^2 p^-1 mod R is unique, so (a^2 + m p) / R is one
number whichever way the columns were filled.  lsqr_pair(a, b) = (lsqr(a), lsqr(b)) raw, on neighbours of the list in both orders.

G1 formulas: 64 seeded scalars k_i, P_i = k_i G from the oracle; the expected results are the oracle's own points (k_i + k_j) G and 2 k_i G,
so no formula of the code under test (nor of the Python reference) produces the expectation.  Every formula is fed P + Q, P + P, P + (-P)
and infinity on either side; XYZZ operands carry a random Z, and in loose mode random coordinates are lifted by q."""
import random

import numpy as np

import arith_cases as K
import arith_checks as chk
import arith_ref as A
from ethsnarks_amd import fields as F

M32 = 0xffffffff
LSQR_PAIR = 26                                    # include/zkhip.h, ZK_PROBE_FR / ZK_PROBE_FQ index
N_POINTS = 64


def field_values(p):
    top = (1 << 254) - 1                          # the largest all-ones value below 2p (2^254 < 2p < 2^255)
    v = [0, 1, p - 1, p, p + 1, 2 * p - 1, A.RMONT % p, top]
    v += [(M32 << (32 * k)) & top for k in range(8)]
    alt = sum(M32 << (64 * k) for k in range(4))  # limbs 0, 2, 4, 6
    v += [alt, (alt << 32) & top]
    rng = random.Random(20261)
    v += [rng.randrange(2 * p) for _ in range(256)]
    assert all(0 <= x < 2 * p for x in v) and top < 2 * p < 2 * top
    return v


def _run(zk, field, idx, cases, width):
    base = zk.PROBE_FR if field == "fr" else zk.PROBE_FQ
    return chk._probe(zk, base + idx, [x for t in cases for x in t], width)


def check_lsqr(zk, field):
    p = A.MOD[field]
    vals = field_values(p)
    got = _run(zk, field, K.FIELD_OPS["lsqr"][0], [(a,) for a in vals], 1)
    prod = _run(zk, field, K.FIELD_OPS["lmul"][0], [(a, a) for a in vals], 2)
    ri = A.rinv(p)
    bad = []
    for i, (a, g, m) in enumerate(zip(vals, got, prod)):
        want = a * a * ri % p
        errs = []
        if g[0] % p != want: errs.append("not a^2 R^-1 mod p = %s" % chk._hx(want))
        if g[0] >= 2 * p: errs.append("not below 2p")
        if g[0] % p != m[0] % p: errs.append("canonical form differs from lmul(a, a) = %s" % chk._hx(m[0]))
        if g[0] != m[0]: errs.append("limbs differ from lmul(a, a) = %s" % chk._hx(m[0]))
        if errs:
            bad.append("lsqr %s case %d operand %s: got %s: %s" % (field, i, chk._hx(a), chk._hx(g[0]), "; ".join(errs)))
    chk._report("lsqr over %s (%d cases)" % (field, len(vals)), bad)


def check_lsqr_pair(zk, field):
    p = A.MOD[field]
    vals = field_values(p)
    assert zk.arith_probe_shape((zk.PROBE_FR if field == "fr" else zk.PROBE_FQ) + LSQR_PAIR) == (2, 2)
    single = [g[0] for g in _run(zk, field, K.FIELD_OPS["lsqr"][0], [(a,) for a in vals], 1)]
    n = len(vals)
    bad = []
    for label, idx in (("", [(i, (i + 1) % n) for i in range(n)]), (" (swapped)", [((i + 1) % n, i) for i in range(n)])):
        got = _run(zk, field, LSQR_PAIR, [(vals[i], vals[j]) for i, j in idx], 2)
        for c, ((i, j), g) in enumerate(zip(idx, got)):
            if g != [single[i], single[j]]:
                bad.append("lsqr_pair%s %s case %d operands %s: got %s, lsqr gives %s" % (label, field, c, chk._hx((vals[i], vals[j])), chk._hx(tuple(g)),
                                                                                       chk._hx((single[i], single[j]))))
    chk._report("lsqr_pair against lsqr over %s (%d pairs, both orders)" % (field, n), bad)


# ---------------------------------------------------------------- G1 formulas against the oracle's points
_cache = {}


def _oracle_points(oracle):
    """scalars k_i and the oracle's k_i G, (k_i + k_{i+1}) G, 2 k_i G as canonical affine integers; computed once"""
    if "pts" not in _cache:
        rng = random.Random(20262)
        ks = [rng.randrange(1, A.FR) for _ in range(N_POINTS)]
        aff = lambda sc: [tuple(F.fq_from_mont(row.reshape(2, 4))) for row in oracle.batch_mul(F.fr_to_mont(sc))]
        _cache["pts"] = (aff(ks), aff([(ks[i] + ks[(i + 1) % N_POINTS]) % A.FR for i in range(N_POINTS)]), aff([2 * k % A.FR for k in ks]))
    return _cache["pts"]


def g1_cases(name, oracle, loose):
    """[(label, operands, expected affine point or None)]"""
    P, S, D = _oracle_points(oracle)
    b = K._CurveBuilder(False, loose, seed=300 + K.CURVE_OPS[name])
    shape = K.CURVE_SHAPE[name]
    pat = lambda: b.rng.getrandbits(16) if loose else 0
    X = lambda pt: b.raw(b.xyzz(pt, b.felem()), pat())
    Af = lambda pt: b.raw(pt, pat())
    cases = []
    for i in range(N_POINTS):
        Pi, Qi = P[i], P[(i + 1) % N_POINTS]
        if shape == "A":
            cases.append(("2P affine", (Af(Pi),), D[i]))
        elif shape == "X":
            cases.append(("2P", (X(Pi),), D[i]))
        else:
            other = Af if shape == "XA" else X
            cases.append(("P + Q", (X(Pi), other(Qi)), S[i]))
            cases.append(("P + P", (X(Pi), other(Pi)), D[i]))
            cases.append(("P + (-P)", (X(Pi), other(b.neg(Pi))), None))
    inf_x, inf_a = b.infinities_x(), b.infinities_a()
    if shape == "A":
        cases += [("affine infinity", (a,), None) for a in inf_a]
    elif shape == "X":
        cases += [("infinity", (x,), None) for x in inf_x]
    else:
        inf_o = inf_a if shape == "XA" else inf_x
        other = Af if shape == "XA" else X
        for x in inf_x:
            cases.append(("infinity + Q", (x, other(P[2])), P[2]))
            cases += [("infinity + infinity", (x, o), None) for o in inf_o]
        cases += [("P + infinity", (X(P[3]), o), P[3]) for o in inf_o]
    return cases


def check_g1_formula(zk, oracle, name, loose):
    ref = A.CurveRef(False)
    cases = g1_cases(name, oracle, loose)
    got = chk.run_curve(zk, False, name, [(label, ops) for label, ops, _ in cases])
    bad = []
    for i, ((label, ops, want), res) in enumerate(zip(cases, got)):
        errs = chk._point_errors(ref, res[0], want, 2 * A.FQ)
        if errs:
            bad.append("G1 %s case %d (%s) operands %s: got %s: %s" % (name, i, label, chk._show(ops), chk._hx(res[0]), "; ".join(errs)))
    chk._report("G1 %s against the oracle's points (%d cases)" % (name, len(cases)), bad)


G1_FORMULAS = ["madd", "madd_pairs", "dbl", "dbl_affine", "add"]


def premises():
    """from the lists alone: the field list holds what the issue names, and the formula lists hold every exceptional case"""
    for p in (A.FR, A.FQ):
        v = field_values(p)
        assert {0, 1, p - 1, p, p + 1, 2 * p - 1, A.RMONT % p, (1 << 254) - 1} <= set(v) and len(v) == 8 + 8 + 2 + 256
        assert all(any(x == (M32 << (32 * k)) for x in v) for k in range(7)) and (0x3fffffff << 224) in v
        limbs = lambda x: [(x >> (32 * k)) & M32 for k in range(8)]
        assert any(limbs(x)[0:7] == [M32, 0] * 3 + [M32] for x in v) and any(limbs(x)[0:7] == [0, M32] * 3 + [0] for x in v)
