"""What the arithmetic-probe tests assert, shared by test_arith_emul.py and test_arith_gpu.py: every check takes the binding (`zk`, the
emulation library or the device library loaded into ethsnarks_amd.prover) and compares zk.arith_probe with tests/arith_ref.py over the
lists of tests/arith_cases.py.

The assertions are contracts -- the value mod p, the range of the representative, which representative of zero is allowed -- never the
particular limbs of one implementation.  No case is skipped or filtered; a mismatch names op, field, case index and operands in hex."""
import numpy as np
from ethsnarks_amd import fields as F
import arith_ref as A
import arith_cases as K

MAX_SHOWN = 5


def _hx(v):
    if isinstance(v, tuple):
        return "(" + ", ".join(_hx(x) for x in v) + ")"
    return "0x%064x" % v


def _report(what, failures):
    assert not failures, "%s: %d case(s) fail, the first:\n  " % (what, len(failures)) + "\n  ".join(failures[:MAX_SHOWN])


def _probe(zk, op, flat_ints, words_in):
    """flat_ints: n * words_in raw integers -> list of n lists of result words (raw integers)"""
    n = len(flat_ints) // words_in
    out = zk.arith_probe(op, F.ints_to_limbs(flat_ints).reshape(n, words_in, 4))
    wo = out.shape[1]
    flat = F.limbs_to_ints(out)
    return [flat[i * wo:(i + 1) * wo] for i in range(n)]


def run_field(zk, field, name, cases):
    idx, width, _, _ = K.FIELD_OPS[name]
    base = zk.PROBE_FR if field == "fr" else zk.PROBE_FQ
    assert zk.arith_probe_shape(base + idx) == (width, K.FIELD_OPS[name][2])
    return _probe(zk, base + idx, [v for t in cases for v in t], width)


# ---------------------------------------------------------------- prime fields
def check_field_op(zk, field, name, loose):
    """strict ops: result = reference mod p and < p; loose ops: = reference mod p and < 2p; lis_zero: the boolean; lneg_op: on the device
    the raw result is the integer 2p - a exactly (in the emulation lneg_op is lneg: the loose contract)"""
    p = A.MOD[field]
    cases = K.field_cases(name, p, loose)
    got = run_field(zk, field, name, cases)
    bound = p if name in K.STRICT_RESULT else 2 * p
    bad = []
    for i, (t, g) in enumerate(zip(cases, got)):
        exp = A.field_expected(name, p, t)
        if name == "lis_zero":
            ok = g == exp
        elif name == "lneg_op" and loose:
            ok = g == [2 * p - t[0]]
        else:
            ok = all(gv % p == ev and gv < bound for gv, ev in zip(g, exp))
        if not ok:
            bad.append("%s %s case %d operands %s: got %s, want %s (mod p) below %s" % (name, field, i, _hx(t), _hx(tuple(g)), _hx(tuple(exp)), "p" if bound == p else "2p"))
    _report("%s over %s (%d cases)" % (name, field, len(cases)), bad)


def check_field_x2(zk, field, name, loose):
    """lmul_x2 / lmul2_x2: each output equals the single-product form on the same operands, also with the two operand groups swapped"""
    p = A.MOD[field]
    single = {"lmul_x2": "lmul", "lmul2_x2": "lmul2"}[name]
    cases = K.field_cases(name, p, loose)
    h = K.FIELD_OPS[name][1] // 2
    first = run_field(zk, field, single, [t[:h] for t in cases])
    second = run_field(zk, field, single, [t[h:] for t in cases])
    bad = []
    for label, cs, want in (("", cases, zip(first, second)), (" (groups swapped)", [t[h:] + t[:h] for t in cases], zip(second, first))):
        got = run_field(zk, field, name, cs)
        for i, (t, g, (w0, w1)) in enumerate(zip(cs, got, want)):
            if g != [w0[0], w1[0]]:
                bad.append("%s%s %s case %d operands %s: got %s, %s gives %s" % (name, label, field, i, _hx(t), _hx(tuple(g)), single, _hx((w0[0], w1[0]))))
    _report("%s against %s over %s" % (name, single, field), bad)


def check_reference_against_oracle(oracle, field):
    """the Python reference and the oracle's own C arithmetic pin each other: Montgomery products of the canonical cases"""
    p = A.MOD[field]
    cases = K.binary_cases(p, loose=False)
    a = F.ints_to_limbs([t[0] for t in cases]); b = F.ints_to_limbs([t[1] for t in cases])
    o = np.zeros_like(a)
    fn = oracle.lib().orc_fr_mul if field == "fr" else oracle.lib().orc_fq_mul
    fn(oracle._p64(o), oracle._p64(a), oracle._p64(b), len(cases))
    want = [A.field_expected("mul", p, t)[0] for t in cases]
    bad = ["mul %s case %d operands %s: oracle %s, Python %s" % (field, i, _hx(t), _hx(g), _hx(w))
           for i, (t, g, w) in enumerate(zip(cases, F.limbs_to_ints(o), want)) if g != w]
    _report("oracle product against the Python reference over %s" % field, bad)


# ---------------------------------------------------------------- Fq2
def check_fq2_op(zk, name, loose):
    q = A.FQ
    cases = K.fq2_cases(name, loose)
    width = len(cases[0])
    assert zk.arith_probe_shape(zk.PROBE_FQ2 + K.FQ2_OPS[name]) == (2 * width, 2)
    got = _probe(zk, zk.PROBE_FQ2 + K.FQ2_OPS[name], [c for t in cases for e in t for c in e], 2 * width)
    bad = []
    for i, (t, g) in enumerate(zip(cases, got)):
        exp = A.fq2_expected(name, t)
        if name in K.FQ2_FLAG:
            ok = g == [exp, 0]
        elif name in K.FQ2_STRICT_RESULT:
            ok = tuple(g) == exp
        else:
            ok = (g[0] % q, g[1] % q) == exp and g[0] < 2 * q and g[1] < 2 * q
        if not ok:
            bad.append("fq2 %s case %d operands %s: got %s, want %s (mod q) below %s" % (name, i, _hx(t), _hx(tuple(g)), _hx(exp) if name not in K.FQ2_FLAG else exp,
                                                                                         "q" if name in K.FQ2_STRICT_RESULT else "2q"))
    _report("fq2 %s (%d cases)" % (name, len(cases)), bad)


# ---------------------------------------------------------------- curves
def _flatten_point(pt, g2):
    return [c for v in pt for c in (v if g2 else (v,))]


def run_curve(zk, g2, name, cases):
    """-> per case the list of result points; a point is a tuple of raw coordinates (G2: (c0, c1) pairs)"""
    ew = 2 if g2 else 1
    op = (zk.PROBE_G2 if g2 else zk.PROBE_G1) + K.CURVE_OPS[name]
    wi, wo = zk.arith_probe_shape(op)
    flat = [c for _, operands in cases for pt in operands for c in _flatten_point(pt, g2)]
    assert len(flat) == wi * len(cases)
    out = _probe(zk, op, flat, wi)
    pw = (2 if name == "to_affine" else 4) * ew
    res = []
    for o in out:
        coords = [tuple(o[k:k + 2]) for k in range(0, len(o), 2)] if g2 else o
        per = pw // ew
        res.append([tuple(coords[k:k + per]) for k in range(0, len(coords), per)])
    return res


def _point_errors(ref, pt, want, bound):
    """XYZZ result against the reference's affine point: range, infinity exactly when the reference is, else ZZ != 0, ZZ^3 = ZZZ^2,
    X = x ZZ, Y = y ZZZ (mod q)"""
    errs = []
    if any(c >= bound for c in _flatten_point(pt, ref.g2)):
        errs.append("a coordinate is not below %s" % ("q" if bound == A.FQ else "2q"))
    Xc, Yc, ZZ, ZZZ = [ref.dm(v) for v in pt]
    if ref.is_zero(ZZ) != (want is None):
        errs.append("result is %sinfinity, the reference sum is %s" % ("" if ref.is_zero(ZZ) else "not ", "infinity" if want is None else "a finite point"))
    elif want is not None:
        m = ref.mul
        if m(m(ZZ, ZZ), ZZ) != m(ZZZ, ZZZ): errs.append("ZZ^3 != ZZZ^2")
        if Xc != m(want[0], ZZ): errs.append("X != x ZZ")
        if Yc != m(want[1], ZZZ): errs.append("Y != y ZZZ")
    return errs


def _same_point(ref, a, b):
    ca, cb = [ref.dm(v) for v in a], [ref.dm(v) for v in b]
    if ref.is_zero(ca[2]) or ref.is_zero(cb[2]):
        return ref.is_zero(ca[2]) and ref.is_zero(cb[2])
    m = ref.mul
    return m(ca[0], cb[2]) == m(cb[0], ca[2]) and m(ca[1], cb[3]) == m(cb[1], ca[3])


def _show(operands):
    return "; ".join(_hx(tuple(pt)) for pt in operands)


def check_curve_op(zk, oracle, g2, name, loose):
    ref = A.CurveRef(g2)
    q = A.FQ
    cases = K.curve_cases(name, K.curve_points(oracle, g2), g2, loose)
    got = run_curve(zk, g2, name, cases)
    plain = {"dbl_q": "dbl", "add_q": "add", "madd_q": "madd", "madd_pairs": "madd"}.get(name)
    got_plain = run_curve(zk, g2, plain, cases) if plain else None
    curve = "G2" if g2 else "G1"
    bad = []
    for i, ((label, operands), res) in enumerate(zip(cases, got)):
        want = ref.expected(name, operands)
        errs = []
        if name == "to_affine":
            exp = tuple(ref.mont(v) for v in want) if want is not None else (((0, 0), (0, 0)) if g2 else (0, 0))
            if res[0] != exp: errs.append("not the canonical affine point %s" % _hx(exp))
        elif name == "canon":
            exp = tuple((tuple(c % q for c in v) if g2 else v % q) for v in operands[0])
            if res[0] != exp: errs.append("not the input reduced into [0, q)")
        else:
            if name.endswith("_q") and any(r != res[0] for r in res[1:]):
                errs.append("the four lanes differ: %s" % _show(res))
            errs += _point_errors(ref, res[0], want, 2 * q)
            if plain and not _same_point(ref, res[0], got_plain[i][0]):
                errs.append("not the point %s gives: %s" % (plain, _hx(got_plain[i][0])))
            if name == "madd_pairs" and [ref.dm(v) for v in res[0]] != [ref.dm(v) for v in got_plain[i][0]]:
                errs.append("coordinates differ (mod q) from madd's: %s" % _hx(got_plain[i][0]))
        if errs:
            bad.append("%s %s case %d (%s) operands %s: got %s: %s" % (curve, name, i, label, _show(operands), _hx(res[0]), "; ".join(errs)))
    _report("%s %s (%d cases)" % (curve, name, len(cases)), bad)


# ---------------------------------------------------------------- every raw output, for comparing two builds of the library
def all_raw_outputs(zk, oracle, loose):
    """{key: uint64 array} of the raw probe results over the whole field and curve case list"""
    out = {}
    for field in ("fr", "fq"):
        p = A.MOD[field]
        for name in K.FIELD_OPS:
            out["%s.%s" % (field, name)] = F.ints_to_limbs([v for r in run_field(zk, field, name, K.field_cases(name, p, loose)) for v in r])
    for name in K.FQ2_OPS:
        cases = K.fq2_cases(name, loose)
        res = _probe(zk, zk.PROBE_FQ2 + K.FQ2_OPS[name], [c for t in cases for e in t for c in e], 2 * len(cases[0]))
        out["fq2.%s" % name] = F.ints_to_limbs([v for r in res for v in r])
    for g2 in (False, True):
        pts = K.curve_points(oracle, g2)
        for name in K.CURVE_OPS:
            res = run_curve(zk, g2, name, K.curve_cases(name, pts, g2, loose))
            out["%s.%s" % ("g2" if g2 else "g1", name)] = F.ints_to_limbs([c for r in res for pt in r for c in _flatten_point(pt, g2)])
    return out
