"""Reference for the arithmetic probe (zk_arith_probe): plain Python integers, written from the definitions -- nothing here is
imported from or transcribed out of csrc/bn254.hpp.

Field elements travel as raw 256-bit integers (8 x u32 limbs).  A Montgomery operand v stands for v R^-1 mod p with R = 2^256, so the
Montgomery product of a and b is a b R^-1 mod p.  Expected values are always the mathematical value mod p: which representative of it an
implementation may return ([0, p) or [0, 2p)) is a range assertion of the test, not part of the expected value.

redc_exact() is the integer (T + m p) / 2^256 that Montgomery reduction of T leaves BEFORE any conditional subtraction.  It is used only
to CLASSIFY cases (how many folds by 2p a sum of products needs), never as an expected output.

Group results come from oracle/pyref.py's affine g1_add / g2_add on the affine meaning of the inputs."""
import pyref

FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
assert (FR, FQ) == (pyref.R, pyref.Q)
RBITS = 256
RMONT = 1 << RBITS
MOD = {"fr": FR, "fq": FQ}


def rinv(p):
    return pow(RMONT, -1, p)


def to_mont(p, v):
    return v * RMONT % p


def from_mont(p, v):
    return v * rinv(p) % p


def redc_exact(p, T):
    """(T + m p) / R with m = -T p^-1 mod R: the unreduced output of Montgomery reduction (word-serial or not: m is unique)"""
    m = (-T * pow(p, -1, RMONT)) % RMONT
    v, rem = divmod(T + m * p, RMONT)
    assert rem == 0
    return v


def dot_exact(p, ops, neg_slots=()):
    """exact REDC value of ops[0] ops[1] + ops[2] ops[3] + ..., the operands in neg_slots entering as 2p - operand"""
    o = [2 * p - v if i in neg_slots else v for i, v in enumerate(ops)]
    return redc_exact(p, sum(o[i] * o[i + 1] for i in range(0, len(o), 2)))


def dot_value(p, ops, neg_slots=()):
    """sum of Montgomery products mod p, the operands in neg_slots negated"""
    o = [-v if i in neg_slots else v for i, v in enumerate(ops)]
    return sum(o[i] * o[i + 1] for i in range(0, len(o), 2)) * rinv(p) % p


# ---- expected value (mod p) of the single-result field primitives, by name; operands are raw integers
def field_expected(name, p, a):
    ri = rinv(p)
    if name == "add" or name == "ladd": return [(a[0] + a[1]) % p]
    if name == "sub" or name == "lsub": return [(a[0] - a[1]) % p]
    if name == "neg" or name == "lneg" or name == "lneg_op": return [(-a[0]) % p]
    if name == "mul" or name == "lmul": return [a[0] * a[1] * ri % p]
    if name == "reduce_once" or name == "canon": return [a[0] % p]
    if name == "lsqr": return [a[0] * a[0] * ri % p]
    if name == "ldbl": return [2 * a[0] % p]
    if name == "lis_zero": return [1 if a[0] % p == 0 else 0]
    if name == "lmul_negop": return [dot_value(p, a, (1,))]
    if name == "lmul2": return [dot_value(p, a)]
    if name == "lmul2_negop": return [dot_value(p, a, (3,))]
    if name == "lmul4": return [dot_value(p, a)]
    if name == "lmul4_negop": return [dot_value(p, a, (3, 7))]
    if name == "lmul_x2": return [a[0] * a[1] * ri % p, a[2] * a[3] * ri % p]
    if name == "lmul2_x2": return [dot_value(p, a[:4]), dot_value(p, a[4:])]
    if name == "to_mont": return [a[0] * RMONT % p]
    if name == "from_mont": return [a[0] * ri % p]
    if name == "inv":                                   # the Montgomery form of 1 / (a R^-1); 0 for a = 0 (a^(p-2))
        v = a[0] * ri % p
        return [pow(v, p - 2, p) * RMONT % p]
    raise KeyError(name)


# ---- Fq2 = Fq[u] / (u^2 + 1); elements are (c0, c1) raw Montgomery integers
def _f2_demont(a):
    return (from_mont(FQ, a[0]), from_mont(FQ, a[1]))


def _f2_mont(a):
    return (to_mont(FQ, a[0]), to_mont(FQ, a[1]))


def fq2_expected(name, a):
    """a: list of (c0, c1) pairs; returns the (c0, c1) pair mod q (Montgomery), or 0 / 1 for lis_zero"""
    v = [_f2_demont(x) for x in a]
    if name == "lmul": return _f2_mont(pyref.f2_mul(v[0], v[1]))
    if name == "lsqr": return _f2_mont(pyref.f2_mul(v[0], v[0]))
    if name == "lmul2": return _f2_mont(pyref.f2_add(pyref.f2_mul(v[0], v[1]), pyref.f2_mul(v[2], v[3])))
    if name == "ladd": return _f2_mont(pyref.f2_add(v[0], v[1]))
    if name == "lsub": return _f2_mont(pyref.f2_sub(v[0], v[1]))
    if name == "lis_zero": return 1 if v[0] == (0, 0) else 0
    if name == "ldbl": return _f2_mont(pyref.f2_add(v[0], v[0]))
    if name == "lneg": return _f2_mont(pyref.f2_neg(v[0]))
    if name == "canon": return (a[0][0] % FQ, a[0][1] % FQ)
    if name == "inv": return _f2_mont(pyref.f2_inv(v[0])) if v[0] != (0, 0) else (0, 0)
    if name == "eq": return 1 if v[0] == v[1] else 0
    raise KeyError(name)


# ---- curves.  g2 = False: coordinates are integers mod q; g2 = True: (c0, c1) pairs.  Points arrive in Montgomery form.
class CurveRef:
    def __init__(self, g2):
        self.g2 = g2
        self.add = pyref.g2_add if g2 else pyref.g1_add

    def dm(self, v):                                     # raw Montgomery coordinate -> value mod q
        return _f2_demont(v) if self.g2 else from_mont(FQ, v)

    def mont(self, v):
        return _f2_mont(v) if self.g2 else to_mont(FQ, v)

    def is_zero(self, v):
        return v == (0, 0) if self.g2 else v == 0

    def mul(self, a, b):
        return pyref.f2_mul(a, b) if self.g2 else a * b % FQ

    def inv(self, a):
        return pyref.f2_inv(a) if self.g2 else pow(a, -1, FQ)

    def affine_meaning(self, pt):
        """pt: affine (x, y) or XYZZ (X, Y, ZZ, ZZZ) of raw Montgomery coordinates -> pyref point (None = infinity)"""
        c = [self.dm(v) for v in pt]
        if len(c) == 2:
            return None if self.is_zero(c[0]) and self.is_zero(c[1]) else (c[0], c[1])
        if self.is_zero(c[2]):
            return None
        return (self.mul(c[0], self.inv(c[2])), self.mul(c[1], self.inv(c[3])))

    def expected(self, name, operands):
        pts = [self.affine_meaning(o) for o in operands]
        if name in ("dbl_affine", "dbl", "dbl_q"):
            return self.add(pts[0], pts[0])
        if name in ("madd", "madd_pairs", "madd_q", "add", "add_q"):
            return self.add(pts[0], pts[1])
        if name in ("canon", "to_affine"):
            return pts[0]
        raise KeyError(name)
