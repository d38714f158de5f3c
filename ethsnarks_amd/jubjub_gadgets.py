"""In-circuit Baby JubJub: the reference's point gadgets restated over gadgets.Protoboard, and the MiMC-EdDSA verification circuit composed of
them.  Host-side circuit authoring like gadgets.py; the device fills the witness of the composed circuit (csrc/jubjub.hpp, k_eddsa_fill).

    lookup_1bit_gadget, lookup_2bit_gadget       src/gadgets/lookup_1bit.cpp, lookup_2bit.cpp
    field2bits_strict                            src/gadgets/field2bits_strict.cpp
    IsNonZero                                    src/gadgets/isnonzero.cpp
    ConditionalPoint, PointAdder, PointDoubler   src/jubjub/conditional_point.cpp, adder.cpp, doubler.cpp
    IsOnCurve, NotLowOrder, PointValidator       src/jubjub/isoncurve.cpp, notloworder.cpp, validator.cpp
    fixed_base_mul, ScalarMult                   src/jubjub/fixed_base_mul.cpp, scalarmult.cpp
    lookup_signed_3bit_gadget                    src/gadgets/lookup_signed_3bit.cpp
    MontgomeryAdder, MontgomeryToEdwards         src/jubjub/montgomery.cpp
    fixed_base_mul_zcash                         src/jubjub/fixed_base_mul_zcash.cpp
    PedersenHash, PedersenHashToBits             src/jubjub/pedersen_hash.cpp

Every class allocates its variables in the order of the C++ constructor and emits its constraints in the order of generate_r1cs_constraints.
The reference has no composed MiMC-EdDSA gadget in C++: eddsa_mimc_circuit has the shape of PureEdDSA (src/jubjub/eddsa.cpp) with the hash of
the Python MiMCEdDSA in the place of the Pedersen hash_RAM, and the composition -- the order of the parts, the booleanity of the bits of s, the
zero IV and the range check of the bits of t -- is this project's own.

eddsa_pure_circuit and eddsa_hash_circuit are the reference's PureEdDSA and EdDSA (src/jubjub/eddsa.cpp) with the windowed Pedersen hash in the
circuit; the device fills the witness of the first (k_eddsa_fill_pure).  What they add to the reference is listed at eddsa_pure_circuit.
"""
import hashlib
from collections import namedtuple

from .fields import FR
from .gadgets import Protoboard, V, lc_add, lc_scale, MiMCe7HashGadget, mimc_constants

JUBJUB_A = 168700
JUBJUB_D = 168696
GENERATOR = (16540640123574156134436876038791482806971768689494387082833631921987005038935,
             20819045374670962167435360035096875258406992893633759881276124905556507972311)
FIELD_BITS = 254                                                # FieldT::size_in_bits()
EDDSA_SEED = b"EdDSA_Verify.RAM"


def _inv(v):
    """libff's inverse(); 0 for 0 (only reached with points that are not on the curve)"""
    v %= FR
    return pow(v, FR - 2, FR) if v else 0


def affine_add(p, q):
    """the affine addition of fixed_base_mul.cpp's table construction and PointAdder's witness"""
    (x1, y1), (x2, y2) = p, q
    eps, delta = x1 * x2 % FR, y1 * y2 % FR
    w = JUBJUB_D * eps * delta % FR
    return ((x1 * y2 + y1 * x2) * _inv(1 + w) % FR, (delta - JUBJUB_A * eps) * _inv(1 - w) % FR)


# ----------------------------------------------------------------------------- lookups, bits
class Lookup1bit:
    """lookup_1bit_gadget: r = c[b];  (c0 + b c1 - b c0) * 1 = r"""

    def __init__(self, pb, constants, bit):
        assert len(constants) == 2
        self.pb, self.c, self.b = pb, [int(c) % FR for c in constants], bit
        self.r = pb.allocate()

    def result(self):
        return self.r

    def generate_r1cs_constraints(self):
        c = self.c
        self.pb.add_r1cs_constraint(lc_add(c[0], lc_scale(V(self.b), c[1] - c[0])), 1, V(self.r))

    def generate_r1cs_witness(self):
        self.pb.set_val(self.r, self.c[self.pb.val(self.b)])


class Lookup2bit:
    """lookup_2bit_gadget: r = c[b0 + 2 b1];  (c1 - c0 + b1 (c3 - c2 - c1 + c0)) * b0 = -c0 + r + b1 (c0 - c2)"""

    def __init__(self, pb, constants, bits):
        assert len(constants) == 4 and len(bits) == 2
        self.pb, self.c, self.b = pb, [int(c) % FR for c in constants], list(bits)
        self.r = pb.allocate()

    def result(self):
        return self.r

    def generate_r1cs_constraints(self):
        c, b = self.c, self.b
        lhs = lc_add(c[1] - c[0], lc_scale(V(b[1]), c[3] - c[2] - c[1] + c[0]))
        rhs = lc_add(-c[0], V(self.r), lc_scale(V(b[1]), c[0] - c[2]))
        self.pb.add_r1cs_constraint(lhs, V(b[0]), rhs)

    def generate_r1cs_witness(self):
        self.pb.set_val(self.r, self.c[self.pb.val(self.b[0]) + 2 * self.pb.val(self.b[1])])


class Field2BitsStrict:
    """field2bits_strict: 254 bits (least significant first), the packing gadget with booleanity, 253 `results` and one lookup_1bit per bit
    against the bits of r - 1 (table {0, 1} where that bit is 0, {1, 1} where it is 1); results[i - 1] = comparisons[i - 1] * results[i] from
    the top bit down.  The reference never constrains results[0], and the product of per-bit values is not a comparison: the gadget, restated
    as it is, pins the bits to a value CONGRUENT to the element.  BitsNotAbove below is what makes a decomposition canonical."""

    def __init__(self, pb, element):
        self.pb, self.element = pb, element
        self.bits = pb.allocate_array(FIELD_BITS)
        self.results = pb.allocate_array(FIELD_BITS - 1)
        largest = FR - 1
        self.comparisons = [Lookup1bit(pb, (1, 1) if (largest >> i) & 1 else (0, 1), self.bits[i]) for i in range(FIELD_BITS)]

    def result(self):
        return self.bits

    def generate_r1cs_constraints(self):
        pb = self.pb
        pb.add_r1cs_constraint(1, {b: (1 << i) % FR for i, b in enumerate(self.bits)}, V(self.element))      # packing_gadget, enforce_bitness
        for b in self.bits:
            pb.add_r1cs_constraint(V(b), lc_add(1, lc_scale(V(b), -1)), 0)
        for g in self.comparisons:
            g.generate_r1cs_constraints()
        last = FIELD_BITS - 1
        for i in range(last, 0, -1):
            other = self.comparisons[i].result() if i == last else self.results[i]
            pb.add_r1cs_constraint(V(self.comparisons[i - 1].result()), V(other), V(self.results[i - 1]))

    def generate_r1cs_witness(self, bits_value=None):
        """bits_value: the integer whose bits are written instead of the element's own (a test's non-canonical decomposition)"""
        pb = self.pb
        v = pb.val(self.element) if bits_value is None else int(bits_value)
        for i, b in enumerate(self.bits):
            pb.set_val(b, (v >> i) & 1)
        for g in self.comparisons:
            g.generate_r1cs_witness()
        last = FIELD_BITS - 1
        for i in range(last, 0, -1):
            other = self.comparisons[i].result() if i == last else self.results[i]
            pb.set_val(self.results[i - 1], pb.val(self.comparisons[i - 1].result()) * pb.val(other))


class BitsNotAbove:
    """NOT of the reference: sum 2^i b_i <= c for boolean b (least significant first) and a constant c whose top bit is set.  From the top
    bit down, e = [every higher bit equals that of c]: where c_i = 1, e <- e b_i (a new variable; the top one is b itself); where c_i = 0,
    e b_i = 0.  One constraint per bit below the top, one variable per set bit of c below the top and above its lowest clear bit."""

    def __init__(self, pb, bits, constant):
        n = len(bits)
        assert constant >> (n - 1) == 1
        self.pb, self.bits, self.c = pb, list(bits), constant
        self.lowest_clear = min(i for i in range(n) if not (constant >> i) & 1)
        self.positions = [i for i in range(n - 2, self.lowest_clear, -1) if (constant >> i) & 1]
        self.e = dict(zip(self.positions, pb.allocate_array(len(self.positions))))

    def n_vars(self):
        return len(self.positions)

    def generate_r1cs_constraints(self):
        pb, cur = self.pb, self.bits[-1]
        for i in range(len(self.bits) - 2, self.lowest_clear - 1, -1):
            if (self.c >> i) & 1:
                pb.add_r1cs_constraint(V(cur), V(self.bits[i]), V(self.e[i]))
                cur = self.e[i]
            else:
                pb.add_r1cs_constraint(V(cur), V(self.bits[i]), 0)

    def generate_r1cs_witness(self):
        pb, cur = self.pb, self.pb.val(self.bits[-1])
        for i in self.positions:
            cur = cur * pb.val(self.bits[i]) % FR
            pb.set_val(self.e[i], cur)


class IsNonZero:
    """IsNonZero: Y = [X != 0], M = 1 / X (0 for 0);  Y (1 - Y) = 0,  X (1 - Y) = 0,  X M = Y"""

    def __init__(self, pb, x):
        self.pb, self.x = pb, x
        self.y, self.m = pb.allocate(), pb.allocate()

    def result(self):
        return self.y

    def generate_r1cs_constraints(self):
        pb, not_y = self.pb, lc_add(1, lc_scale(V(self.y), -1))
        pb.add_r1cs_constraint(V(self.y), not_y, 0)
        pb.add_r1cs_constraint(V(self.x), not_y, 0)
        pb.add_r1cs_constraint(V(self.x), V(self.m), V(self.y))

    def generate_r1cs_witness(self):
        x = self.pb.val(self.x)
        self.pb.set_val(self.m, _inv(x))
        self.pb.set_val(self.y, 1 if x else 0)


# ----------------------------------------------------------------------------- points
class ConditionalPoint:
    """ConditionalPoint: (x2, y2) = bit ? (x1, y1) : (0, 1);  x1 bit = x2,  y1 bit = y2 - 1 + bit"""

    def __init__(self, pb, x1, y1, bit):
        self.pb, self.x1, self.y1, self.bit = pb, x1, y1, bit
        self.x2, self.y2 = pb.allocate(), pb.allocate()

    def result_x(self):
        return self.x2

    def result_y(self):
        return self.y2

    def generate_r1cs_constraints(self):
        pb = self.pb
        pb.add_r1cs_constraint(V(self.x1), V(self.bit), V(self.x2))
        pb.add_r1cs_constraint(V(self.y1), V(self.bit), lc_add(V(self.y2), -1, V(self.bit)))

    def generate_r1cs_witness(self):
        pb, bit = self.pb, self.pb.val(self.bit)
        pb.set_val(self.x2, bit * pb.val(self.x1))
        pb.set_val(self.y2, pb.val(self.y1) if bit else 1)


class PointAdder:
    """PointAdder: beta = x1 y2, gamma = y1 x2, delta = y1 y2, epsilon = x1 x2, tau = delta epsilon,
    x3 (1 + d tau) = beta + gamma,  y3 (1 - d tau) = delta - a epsilon.  The outputs enter through the A row of their constraints."""

    def __init__(self, pb, x1, y1, x2, y2):
        self.pb, self.x1, self.y1, self.x2, self.y2 = pb, x1, y1, x2, y2
        self.beta, self.gamma, self.delta, self.epsilon, self.tau, self.x3, self.y3 = pb.allocate_array(7)

    def result_x(self):
        return self.x3

    def result_y(self):
        return self.y3

    def generate_r1cs_constraints(self):
        pb = self.pb
        pb.add_r1cs_constraint(V(self.x1), V(self.y2), V(self.beta))
        pb.add_r1cs_constraint(V(self.y1), V(self.x2), V(self.gamma))
        pb.add_r1cs_constraint(V(self.y1), V(self.y2), V(self.delta))
        pb.add_r1cs_constraint(V(self.x1), V(self.x2), V(self.epsilon))
        pb.add_r1cs_constraint(V(self.delta), V(self.epsilon), V(self.tau))
        pb.add_r1cs_constraint(V(self.x3), lc_add(1, lc_scale(V(self.tau), JUBJUB_D)), lc_add(V(self.beta), V(self.gamma)))
        pb.add_r1cs_constraint(V(self.y3), lc_add(1, lc_scale(V(self.tau), -JUBJUB_D)), lc_add(V(self.delta), lc_scale(V(self.epsilon), -JUBJUB_A)))

    def generate_r1cs_witness(self):
        pb = self.pb
        x1, y1, x2, y2 = pb.val(self.x1), pb.val(self.y1), pb.val(self.x2), pb.val(self.y2)
        beta, gamma, delta, eps = x1 * y2 % FR, y1 * x2 % FR, y1 * y2 % FR, x1 * x2 % FR
        tau = delta * eps % FR
        for var, v in zip((self.beta, self.gamma, self.delta, self.epsilon, self.tau), (beta, gamma, delta, eps, tau)):
            pb.set_val(var, v)
        pb.set_val(self.x3, (beta + gamma) * _inv(1 + JUBJUB_D * tau))
        pb.set_val(self.y3, (delta - JUBJUB_A * eps) * _inv(1 - JUBJUB_D * tau))


class PointDoubler:
    """PointDoubler: alpha = x x, beta = y y, gamma = d alpha beta, delta = 2 x y,  (gamma + 1) x3 = delta,  (gamma - 1) y3 = a alpha - beta.
    The outputs enter through the B row of their constraints."""

    def __init__(self, pb, x1, y1):
        self.pb, self.x1, self.y1 = pb, x1, y1
        self.alpha, self.beta, self.gamma, self.delta, self.x3, self.y3 = pb.allocate_array(6)

    def result_x(self):
        return self.x3

    def result_y(self):
        return self.y3

    def generate_r1cs_constraints(self):
        pb = self.pb
        pb.add_r1cs_constraint(V(self.x1), V(self.x1), V(self.alpha))
        pb.add_r1cs_constraint(V(self.y1), V(self.y1), V(self.beta))
        pb.add_r1cs_constraint(lc_scale(V(self.alpha), JUBJUB_D), V(self.beta), V(self.gamma))
        pb.add_r1cs_constraint(lc_scale(V(self.x1), 2), V(self.y1), V(self.delta))
        pb.add_r1cs_constraint(lc_add(V(self.gamma), 1), V(self.x3), V(self.delta))
        pb.add_r1cs_constraint(lc_add(V(self.gamma), -1), V(self.y3), lc_add(lc_scale(V(self.alpha), JUBJUB_A), lc_scale(V(self.beta), -1)))

    def generate_r1cs_witness(self):
        pb = self.pb
        x, y = pb.val(self.x1), pb.val(self.y1)
        alpha, beta = x * x % FR, y * y % FR
        gamma, delta = JUBJUB_D * alpha * beta % FR, 2 * x * y % FR
        for var, v in zip((self.alpha, self.beta, self.gamma, self.delta), (alpha, beta, gamma, delta)):
            pb.set_val(var, v)
        pb.set_val(self.x3, delta * _inv(gamma + 1))
        pb.set_val(self.y3, (JUBJUB_A * alpha - beta) * _inv(gamma - 1))


class IsOnCurve:
    """IsOnCurve: xx = x x, yy = y y,  d xx yy = a xx + yy - 1"""

    def __init__(self, pb, x, y):
        self.pb, self.x, self.y = pb, x, y
        self.xx, self.yy = pb.allocate(), pb.allocate()

    def generate_r1cs_constraints(self):
        pb = self.pb
        pb.add_r1cs_constraint(V(self.x), V(self.x), V(self.xx))
        pb.add_r1cs_constraint(V(self.y), V(self.y), V(self.yy))
        pb.add_r1cs_constraint(lc_scale(V(self.xx), JUBJUB_D), V(self.yy), lc_add(lc_scale(V(self.xx), JUBJUB_A), V(self.yy), -1))

    def generate_r1cs_witness(self):
        x, y = self.pb.val(self.x), self.pb.val(self.y)
        self.pb.set_val(self.xx, x * x)
        self.pb.set_val(self.yy, y * y)


class NotLowOrder:
    """NotLowOrder: three doublings, IsNonZero of the x of 8 P, and  result * 1 = 1"""

    def __init__(self, pb, x, y):
        self.pb = pb
        self.doublers = [PointDoubler(pb, x, y)]
        for _ in range(2):
            self.doublers.append(PointDoubler(pb, self.doublers[-1].result_x(), self.doublers[-1].result_y()))
        self.isnonzero = IsNonZero(pb, self.doublers[-1].result_x())

    def generate_r1cs_constraints(self):
        for g in self.doublers:
            g.generate_r1cs_constraints()
        self.isnonzero.generate_r1cs_constraints()
        self.pb.add_r1cs_constraint(V(self.isnonzero.result()), 1, 1)

    def generate_r1cs_witness(self):
        for g in self.doublers:
            g.generate_r1cs_witness()
        self.isnonzero.generate_r1cs_witness()


class PointValidator:
    """PointValidator: NotLowOrder is allocated first, IsOnCurve constrained first"""

    def __init__(self, pb, x, y):
        self.notloworder = NotLowOrder(pb, x, y)
        self.isoncurve = IsOnCurve(pb, x, y)

    def generate_r1cs_constraints(self):
        self.isoncurve.generate_r1cs_constraints()
        self.notloworder.generate_r1cs_constraints()

    def generate_r1cs_witness(self):
        self.isoncurve.generate_r1cs_witness()
        self.notloworder.generate_r1cs_witness()


def fixed_base_table(base, n_windows):
    """the lookup tables of fixed_base_mul: window i holds [(0, 1), P, 2 P, 3 P] with P = 4^i base, by the constructor's chain of affine additions"""
    rows, start, cur = [], base, base
    for _ in range(n_windows):
        row = [(0, 1)]
        for _j in range(1, 4):
            row.append(cur)
            cur = affine_add(start, cur)
        rows.append(row)
        start = cur
    return rows


class FixedBaseMul:
    """fixed_base_mul: 2-bit windows over a constant base point.  Per window a lookup_2bit for x and one for y (allocated in turn), then the
    adders: the first adds windows 0 and 1, adder i the previous sum and window i + 1.  Constraints: the x lookups, the y lookups, the adders."""

    def __init__(self, pb, base, scalar_bits):
        assert len(scalar_bits) % 2 == 0 and len(scalar_bits) >= 4
        n_windows = len(scalar_bits) // 2
        self.table = fixed_base_table((int(base[0]) % FR, int(base[1]) % FR), n_windows)
        self.windows_x, self.windows_y, self.adders = [], [], []
        for i, row in enumerate(self.table):
            bits = scalar_bits[2 * i:2 * i + 2]
            self.windows_x.append(Lookup2bit(pb, [p[0] for p in row], bits))
            self.windows_y.append(Lookup2bit(pb, [p[1] for p in row], bits))
        for i in range(1, n_windows):
            px, py = (self.windows_x[0].result(), self.windows_y[0].result()) if i == 1 else (self.adders[-1].result_x(), self.adders[-1].result_y())
            self.adders.append(PointAdder(pb, px, py, self.windows_x[i].result(), self.windows_y[i].result()))

    def result_x(self):
        return self.adders[-1].result_x()

    def result_y(self):
        return self.adders[-1].result_y()

    def generate_r1cs_constraints(self):
        for g in self.windows_x + self.windows_y + self.adders:
            g.generate_r1cs_constraints()

    def generate_r1cs_witness(self):
        for g in self.windows_x + self.windows_y + self.adders:
            g.generate_r1cs_witness()


class ScalarMult:
    """ScalarMult (variable base): conditionals[0] on the point itself, then per further bit a doubler, a conditional and an adder, allocated
    in turn (15 variables a bit).  Constraints: every doubler, every conditional, every adder."""

    def __init__(self, pb, x, y, scalar_bits):
        assert len(scalar_bits) > 1
        self.conditionals = [ConditionalPoint(pb, x, y, scalar_bits[0])]
        self.doublers, self.adders = [], []
        for i in range(1, len(scalar_bits)):
            px, py = (x, y) if i == 1 else (self.doublers[-1].result_x(), self.doublers[-1].result_y())
            dbl = PointDoubler(pb, px, py)
            self.doublers.append(dbl)
            cond = ConditionalPoint(pb, dbl.result_x(), dbl.result_y(), scalar_bits[i])
            self.conditionals.append(cond)
            prev = self.conditionals[0] if i == 1 else self.adders[-1]
            self.adders.append(PointAdder(pb, prev.result_x(), prev.result_y(), cond.result_x(), cond.result_y()))

    def result_x(self):
        return self.adders[-1].result_x()

    def result_y(self):
        return self.adders[-1].result_y()

    def generate_r1cs_constraints(self):
        for g in self.doublers + self.conditionals + self.adders:
            g.generate_r1cs_constraints()

    def generate_r1cs_witness(self):
        for g in self.doublers + self.conditionals + self.adders:
            g.generate_r1cs_witness()


# ----------------------------------------------------------------------------- the MiMC-EdDSA circuit
LAYOUT_FIELDS = ("msg_len", "n_vars", "ax_var", "msg_var0", "rx_var", "s_bit0", "iv_var", "validator_var0", "window_var0", "fixed_adder_var0",
                 "mimc_var0", "t_bit0", "t_range_var0", "cond0_var", "doubler_var0", "cond_var0", "adder_var0", "step_stride", "last_adder_var0")
EddsaLayout = namedtuple("EddsaLayout", LAYOUT_FIELDS)
EddsaLayout.__doc__ = """Where the segments of a witness row of eddsa_mimc_circuit start (variable indices; variable 0 is ONE; a row has n_vars + 1 elements):
    ax_var            A.x, A.y                                                   (public)
    msg_var0          msg_len message elements                                   (public)
    rx_var            R.x, R.y
    s_bit0            the 254 bits of s, least significant first
    iv_var            the zero IV of the hash
    validator_var0    3 x (alpha, beta, gamma, delta, x3, y3) of the doublings of R, then Y, M of IsNonZero, then xx, yy of IsOnCurve: 22
    window_var0       127 x (x, y) of the 2-bit lookups                          stride 2
    fixed_adder_var0  126 x (beta, gamma, delta, epsilon, tau, x3, y3)           stride 7
    mimc_var0         4 + msg_len outputs, then per hashed element 91 x (a, b, c, d)
    t_bit0            the 254 bits of t, the 253 results, the 254 comparisons of field2bits_strict
    t_range_var0      the running products of BitsNotAbove(bits of t, r - 1), from the top bit down
    cond0_var         (x2, y2) of conditionals[0]
    doubler_var0, cond_var0, adder_var0   the 6, 2, 7 variables of step i = 1 .. 253 of the variable-base multiplication at + (i - 1) step_stride
    last_adder_var0   the 7 variables of R + t A"""

N_S_BITS = FIELD_BITS
N_WINDOWS = N_S_BITS // 2


class EddsaMimcCircuit:
    """The gadgets of eddsa_mimc_circuit on one protoboard; assign() writes another signature's witness into the same constraint system"""

    def __init__(self, msg_len=1, B=None):
        assert msg_len >= 1
        self.msg_len, self.B = int(msg_len), tuple(B) if B is not None else GENERATOR
        pb = self.pb = Protoboard()
        self.ax, self.ay = pb.allocate(), pb.allocate()
        self.msg = pb.allocate_array(self.msg_len)
        pb.set_input_sizes(2 + self.msg_len)
        self.rx, self.ry = pb.allocate(), pb.allocate()
        self.s_bits = pb.allocate_array(N_S_BITS)
        self.iv = pb.allocate()
        mark = lambda: len(pb.values)
        at = {}
        at["validator_var0"] = mark()
        self.validator = PointValidator(pb, self.rx, self.ry)
        at["window_var0"] = mark()
        self.lhs = FixedBaseMul(pb, self.B, self.s_bits)
        at["fixed_adder_var0"] = self.lhs.adders[0].beta
        at["mimc_var0"] = mark()
        self.hash = MiMCe7HashGadget(pb, self.iv, [self.rx, self.ry, self.ax, self.ay] + self.msg, constants=mimc_constants(seed=EDDSA_SEED))
        at["t_bit0"] = mark()
        self.t_bits = Field2BitsStrict(pb, self.hash.result())
        at["t_range_var0"] = mark()
        self.t_range = BitsNotAbove(pb, self.t_bits.result(), FR - 1)
        at["cond0_var"] = mark()
        self.at = ScalarMult(pb, self.ax, self.ay, self.t_bits.result())
        at["last_adder_var0"] = mark()
        self.rhs = PointAdder(pb, self.rx, self.ry, self.at.result_x(), self.at.result_y())
        sm = self.at
        self.layout = EddsaLayout(msg_len=self.msg_len, n_vars=len(pb.values) - 1, ax_var=self.ax, msg_var0=self.msg[0], rx_var=self.rx,
                                  s_bit0=self.s_bits[0], iv_var=self.iv, doubler_var0=sm.doublers[0].alpha, cond_var0=sm.conditionals[1].x2,
                                  adder_var0=sm.adders[0].beta, step_stride=sm.doublers[1].alpha - sm.doublers[0].alpha, **at)
        # constraints: the inputs' own, then the parts in the order of PureEdDSA::generate_r1cs_constraints
        for b in self.s_bits:
            pb.add_r1cs_constraint(V(b), lc_add(1, lc_scale(V(b), -1)), 0)
        pb.add_r1cs_constraint(V(self.iv), 1, 0)
        self.validator.generate_r1cs_constraints()
        self.lhs.generate_r1cs_constraints()
        self.hash.generate_r1cs_constraints()
        self.t_bits.generate_r1cs_constraints()
        self.t_range.generate_r1cs_constraints()
        self.at.generate_r1cs_constraints()
        self.rhs.generate_r1cs_constraints()
        pb.add_r1cs_constraint(V(self.lhs.result_x()), 1, V(self.rhs.result_x()))
        pb.add_r1cs_constraint(V(self.lhs.result_y()), 1, V(self.rhs.result_y()))
        self._r1cs = None

    def r1cs(self):
        if self._r1cs is None:
            self._r1cs = self.pb.to_r1cs()[0]
        return self._r1cs

    def assign(self, A, R, s, msg, t_bits_value=None):
        """generate_r1cs_witness for one signature; returns the witness (a list of n_vars + 1 ints).  s: an integer below 2^254"""
        pb = self.pb
        assert 0 <= s < 1 << N_S_BITS and len(msg) == self.msg_len
        for var, v in zip([self.ax, self.ay] + self.msg + [self.rx, self.ry], [A[0], A[1]] + list(msg) + [R[0], R[1]]):
            pb.set_val(var, int(v))
        for i, b in enumerate(self.s_bits):
            pb.set_val(b, (s >> i) & 1)
        pb.set_val(self.iv, 0)
        self.validator.generate_r1cs_witness()
        self.lhs.generate_r1cs_witness()
        self.hash.generate_r1cs_witness()
        self.t_bits.generate_r1cs_witness(t_bits_value)
        self.t_range.generate_r1cs_witness()
        self.at.generate_r1cs_witness()
        self.rhs.generate_r1cs_witness()
        return list(pb.values)

    def public_inputs(self, A, msg):
        return [int(A[0]) % FR, int(A[1]) % FR] + [int(m) % FR for m in msg]

    def equation_holds(self):
        """the two closing constraints alone: lhs == rhs"""
        pb = self.pb
        return pb.val(self.lhs.result_x()) == pb.val(self.rhs.result_x()) and pb.val(self.lhs.result_y()) == pb.val(self.rhs.result_y())


def eddsa_mimc_circuit(msg_len=1, B=None, A=None, R=None, s=None, msg=None):
    """MiMC-EdDSA verification, S B == R + t A with t = mimc_hash([R.x, R.y, A.x, A.y, M..], 0) under the constants of seed "EdDSA_Verify.RAM":

        1. PointValidator(R)                     2. lhs = FixedBaseMul(B, bits of s), 254 bits
        3. t = MiMC hash, IV 0                   4. Field2BitsStrict(t), and BitsNotAbove(bits, r - 1)
        5. At = ScalarMult(A, bits of t)         6. rhs = PointAdder(R, At)              7. lhs.x == rhs.x, lhs.y == rhs.y

    PUBLIC: A.x, A.y and the msg_len message elements (2 + msg_len inputs).  PRIVATE: R, the bits of s, everything derived.
    Returns (protoboard, EddsaLayout); with A, R, s and msg given the protoboard holds that signature's witness, otherwise all zeros.
    The circuit differs from EdDSAVerifier("mimc") in two places: PointValidator refuses an R of low order (8 R = identity), which the verifier
    accepts; and s enters as 254 bits, so the circuit takes any s below 2^254 where the verifier wants s below r."""
    c = EddsaMimcCircuit(msg_len, B)
    if A is not None:
        c.assign(A, R, s, msg)
    return c.pb, c.layout


# ----------------------------------------------------------------------------- the in-circuit Pedersen hash
MONTGOMERY_A = 168698                                           # Params::A; Params::scale is 1
MONTGOMERY_SCALE = 1
CHUNK_BITS = 3
CHUNKS_PER_BASE_POINT = 62
PEDERSEN_MSG_SEED = b"EdDSA_Verify.M"


def _lc_val(pb, lc):
    return sum(c * pb.values[i] for i, c in Protoboard._lc(lc).items()) % FR


def _sqrt(a):
    """Tonelli-Shanks in Fr; None for a non-residue"""
    a %= FR
    if a == 0:
        return 0
    if pow(a, (FR - 1) // 2, FR) != 1:
        return None
    s, q = 0, FR - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    z = 2
    while pow(z, (FR - 1) // 2, FR) != FR - 1:
        z += 1
    m, c, t, r = s, pow(z, q, FR), pow(a, q, FR), pow(a, (q + 1) // 2, FR)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u, i = u * u % FR, i + 1
        b = pow(c, 1 << (m - i - 1), FR)
        m, c, t, r = i, b * b % FR, t * b * b % FR, r * b % FR
    return r


_BASEPOINTS = {}


def pedersen_basepoint(name, i):
    """EdwardsPoint::make_basepoint(name, i): Point.from_hash of "%-28s%04X" -- y = sha256 mod r, incremented until x^2 = (y^2 - 1) / (d y^2 - a)
    is a square, x the root above r - x, times the cofactor 8.  What zk_jj_pedersen_basepoint computes, here on Python integers"""
    name = name.encode("ascii") if isinstance(name, str) else bytes(name)
    if len(name) > 28 or not 0 <= i <= 0xFFFF:
        raise ValueError("a Pedersen name has at most 28 bytes and a base point index at most 0xFFFF")
    if (name, i) not in _BASEPOINTS:
        y = int.from_bytes(hashlib.sha256(b"%-28s%04X" % (name, i)).digest(), "big") % FR
        while True:
            ysq = y * y % FR
            x = _sqrt((ysq - 1) * _inv(JUBJUB_D * ysq - JUBJUB_A))
            if x is not None:
                break
            y = (y + 1) % FR
        p = (max(x, FR - x), y)
        for _ in range(3):
            p = affine_add(p, p)
        _BASEPOINTS[(name, i)] = p
    return _BASEPOINTS[(name, i)]


def as_montgomery(p):
    """EdwardsPoint::as_montgomery: u = (1 + y) / (1 - y), v = scale u / x"""
    u = (1 + p[1]) * _inv(1 - p[1]) % FR
    return (u, MONTGOMERY_SCALE * u * _inv(p[0]) % FR)


class LookupSigned3bit:
    """lookup_signed_3bit_gadget: r = +-c[b0 + 2 b1], negated when b2.  b0b1 is allocated before r;
    b0 b1 = b0b1,  (2 y_lc) b2 = y_lc - r  with  y_lc = c0 + b0 (c1 - c0) + b1 (c2 - c0) + b0b1 (c3 - c2 - c1 + c0)"""

    def __init__(self, pb, constants, bits):
        assert len(constants) == 4 and len(bits) == 3
        self.pb, self.c, self.b = pb, [int(c) % FR for c in constants], list(bits)
        self.b0b1, self.r = pb.allocate(), pb.allocate()

    def result(self):
        return self.r

    def lc(self, c):
        """the 2-bit lookup of the constants c as a linear combination over b0, b1 and b0b1"""
        return lc_add(c[0], lc_scale(V(self.b[0]), c[1] - c[0]), lc_scale(V(self.b[1]), c[2] - c[0]), lc_scale(V(self.b0b1), c[3] - c[2] - c[1] + c[0]))

    def generate_r1cs_constraints(self):
        pb, y_lc = self.pb, self.lc(self.c)
        pb.add_r1cs_constraint(V(self.b[0]), V(self.b[1]), V(self.b0b1))
        pb.add_r1cs_constraint(lc_scale(y_lc, 2), V(self.b[2]), lc_add(y_lc, lc_scale(V(self.r), -1)))

    def generate_r1cs_witness(self):
        pb = self.pb
        i = pb.val(self.b[0]) + 2 * pb.val(self.b[1]) + 4 * pb.val(self.b[2])
        pb.set_val(self.b0b1, pb.val(self.b[0]) * pb.val(self.b[1]))
        pb.set_val(self.r, -self.c[i & 3] if i > 3 else self.c[i & 3])


class MontgomeryAdder:
    """MontgomeryAdder: lambda, X3, Y3;  (X2 - X1) lambda = Y2 - Y1,  lambda lambda = A + X1 + X2 + X3,  (X1 - X3) lambda = Y3 + Y1.
    X1 and X2 are linear combinations, Y1 and Y2 variables.  X1 == X2 has no witness (the inverse of zero): the caller rules it out"""

    def __init__(self, pb, x1, y1, x2, y2):
        self.pb, self.x1, self.y1, self.x2, self.y2 = pb, Protoboard._lc(x1), y1, Protoboard._lc(x2), y2
        self.lam, self.x3, self.y3 = pb.allocate(), pb.allocate(), pb.allocate()

    def result_x(self):
        return self.x3

    def result_y(self):
        return self.y3

    def generate_r1cs_constraints(self):
        pb, lam = self.pb, V(self.lam)
        pb.add_r1cs_constraint(lc_add(self.x2, lc_scale(self.x1, -1)), lam, lc_add(V(self.y2), lc_scale(V(self.y1), -1)))
        pb.add_r1cs_constraint(lam, lam, lc_add(MONTGOMERY_A, self.x1, self.x2, V(self.x3)))
        pb.add_r1cs_constraint(lc_add(self.x1, lc_scale(V(self.x3), -1)), lam, lc_add(V(self.y3), V(self.y1)))

    def generate_r1cs_witness(self):
        pb = self.pb
        x1, x2, y1, y2 = _lc_val(pb, self.x1), _lc_val(pb, self.x2), pb.val(self.y1), pb.val(self.y2)
        lam = (y2 - y1) * _inv(x2 - x1) % FR
        x3 = (lam * lam - MONTGOMERY_A - x1 - x2) % FR
        pb.set_val(self.lam, lam)
        pb.set_val(self.x3, x3)
        pb.set_val(self.y3, -(y1 + lam * (x3 - x1)))


class MontgomeryToEdwards:
    """MontgomeryToEdwards: x = scale X / Y, y = (X - 1) / (X + 1);  Y x = scale X,  (X + 1) y = X - 1.  X is a linear combination"""

    def __init__(self, pb, x, y):
        self.pb, self.x1, self.y1 = pb, Protoboard._lc(x), y
        self.x2, self.y2 = pb.allocate(), pb.allocate()

    def result_x(self):
        return self.x2

    def result_y(self):
        return self.y2

    def generate_r1cs_constraints(self):
        pb = self.pb
        pb.add_r1cs_constraint(V(self.y1), V(self.x2), lc_scale(self.x1, MONTGOMERY_SCALE))
        pb.add_r1cs_constraint(lc_add(self.x1, 1), V(self.y2), lc_add(self.x1, -1))

    def generate_r1cs_witness(self):
        pb, x = self.pb, _lc_val(self.pb, self.x1)
        pb.set_val(self.x2, MONTGOMERY_SCALE * x * _inv(pb.val(self.y1)))
        pb.set_val(self.y2, (x - 1) * _inv(x + 1))


def zcash_window_table(base_points, n_windows):
    """the Edwards points of fixed_base_mul_zcash's tables: window i holds (1 .. 4) 16^(i % 62) base_points[i / 62], by the constructor's additions"""
    rows = []
    for i in range(n_windows):
        if i % CHUNKS_PER_BASE_POINT == 0:
            start = (int(base_points[i // CHUNKS_PER_BASE_POINT][0]) % FR, int(base_points[i // CHUNKS_PER_BASE_POINT][1]) % FR)
        row, cur = [start], start
        for _ in range(3):
            cur = affine_add(cur, start)
            row.append(cur)
        rows.append(row)
        start = affine_add(cur, cur)
        start = affine_add(start, start)
    return rows


class FixedBaseMulZcash:
    """fixed_base_mul_zcash: 3-bit chunks, 62 to a base point.  Per window a lookup_signed_3bit for the Montgomery y of its four table points
    (b0b1, r) and the Montgomery x as a linear combination over b0, b1, b0b1 (no variable); MontgomeryAdders chain the windows of a segment (the
    first adds windows 0 and 1); one MontgomeryToEdwards per segment; PointAdders chain the converted segments.  Allocation: every window, every
    Montgomery adder, the converters, the Edwards adders.  Constraints: the y lookups, the Montgomery adders, the converters, the Edwards adders.

    The reference's quirk, kept: when the last base point has a single window (n_windows % 62 == 1) its converter is created inside the adder
    loop and therefore stands FIRST in point_converters -- the Edwards chain starts from it.  A single window in all makes the reference read the
    back of an empty vector: fewer than two windows, or a bit count that is no multiple of 3, is a ValueError here.

    No Montgomery adder meets X1 == X2, and no converter a zero denominator, whatever the bits: a window's digit is +-(1 .. 4) 16^j, so the sum
    of the first k windows of a segment is a multiple m B with 0 < |m| < 16^k and window k adds +-(1 .. 4) 16^k B -- equal Montgomery x would
    need m = +-(that digit) mod L, impossible below L; and a segment's sum is a non-zero multiple, below L in absolute value, of a point of
    prime order L, so it is not of low order and neither Y = 0 nor X = -1 (the Montgomery forms of the points of order 2 and 4) occurs."""

    def __init__(self, pb, base_points, scalar_bits):
        n_bits = len(scalar_bits)
        if n_bits % CHUNK_BITS or n_bits < 2 * CHUNK_BITS:
            raise ValueError("fixed_base_mul_zcash takes a multiple of 3 bits and at least two windows, not %d bits" % n_bits)
        n_windows = n_bits // CHUNK_BITS
        if self.basepoints_required(n_bits) > len(base_points):
            raise ValueError("%d bits need %d base points" % (n_bits, self.basepoints_required(n_bits)))
        self.pb, self.n_windows = pb, n_windows
        self.table = zcash_window_table(base_points, n_windows)
        self.windows_x, self.windows_y = [], []
        for i, row in enumerate(self.table):
            mont = [as_montgomery(p) for p in row]
            lut = LookupSigned3bit(pb, [m[1] for m in mont], scalar_bits[3 * i:3 * i + 3])
            self.windows_y.append(lut)
            self.windows_x.append(lut.lc([m[0] for m in mont]))
        self.montgomery_adders, self.point_converters, self.edward_adders = [], [], []
        for i in range(1, n_windows):
            if i % CHUNKS_PER_BASE_POINT == 0:
                if i + 1 < n_windows:
                    continue
                self.point_converters.append(MontgomeryToEdwards(pb, self.windows_x[i], self.windows_y[i].result()))
            elif i % CHUNKS_PER_BASE_POINT == 1:
                self.montgomery_adders.append(MontgomeryAdder(pb, self.windows_x[i - 1], self.windows_y[i - 1].result(), self.windows_x[i], self.windows_y[i].result()))
            else:
                prev = self.montgomery_adders[-1]
                self.montgomery_adders.append(MontgomeryAdder(pb, V(prev.result_x()), prev.result_y(), self.windows_x[i], self.windows_y[i].result()))
        width = CHUNKS_PER_BASE_POINT - 1
        for i in range(width, len(self.montgomery_adders), width):
            a = self.montgomery_adders[i - 1]
            self.point_converters.append(MontgomeryToEdwards(pb, V(a.result_x()), a.result_y()))
        a = self.montgomery_adders[-1]
        self.point_converters.append(MontgomeryToEdwards(pb, V(a.result_x()), a.result_y()))
        for i in range(1, len(self.point_converters)):
            p, q = self.point_converters[i - 1] if i == 1 else self.edward_adders[i - 2], self.point_converters[i]
            self.edward_adders.append(PointAdder(pb, p.result_x(), p.result_y(), q.result_x(), q.result_y()))

    @staticmethod
    def basepoints_required(n_bits):
        return -(-n_bits // (CHUNK_BITS * CHUNKS_PER_BASE_POINT))

    def _last(self):
        return self.edward_adders[-1] if self.edward_adders else self.point_converters[-1]

    def result_x(self):
        return self._last().result_x()

    def result_y(self):
        return self._last().result_y()

    def generate_r1cs_constraints(self):
        for g in self.windows_y + self.montgomery_adders + self.point_converters + self.edward_adders:
            g.generate_r1cs_constraints()

    def generate_r1cs_witness(self):
        for g in self.windows_y + self.montgomery_adders + self.point_converters + self.edward_adders:
            g.generate_r1cs_witness()


class PedersenHash:
    """PedersenHash: fixed_base_mul_zcash over the base points make_basepoints(name, ceil(bits / 186))"""

    def __init__(self, pb, name, bits):
        n = FixedBaseMulZcash.basepoints_required(len(bits))
        self.commitment = FixedBaseMulZcash(pb, [pedersen_basepoint(name, i) for i in range(n)], bits)

    def result_x(self):
        return self.commitment.result_x()

    def result_y(self):
        return self.commitment.result_y()

    def generate_r1cs_constraints(self):
        self.commitment.generate_r1cs_constraints()

    def generate_r1cs_witness(self):
        self.commitment.generate_r1cs_witness()


class PedersenHashToBits:
    """PedersenHashToBits: the hash, then field2bits_strict of its x"""

    def __init__(self, pb, name, bits):
        self.hash = PedersenHash(pb, name, bits)
        self.tobits = Field2BitsStrict(pb, self.hash.result_x())

    def result(self):
        return self.tobits.result()

    def generate_r1cs_constraints(self):
        self.hash.generate_r1cs_constraints()
        self.tobits.generate_r1cs_constraints()

    def generate_r1cs_witness(self, bits_value=None):
        self.hash.generate_r1cs_witness()
        self.tobits.generate_r1cs_witness(bits_value)


# ----------------------------------------------------------------------------- the PureEdDSA and EdDSA circuits
PURE_LAYOUT_FIELDS = ("msg_len", "n_vars", "ax_var", "msg_bit0", "rx_var", "s_bit0", "pad_bit0", "validator_var0", "window_var0", "fixed_adder_var0",
                      "rx_bit0", "rx_range_var0", "ax_bit0", "ax_range_var0", "hash_window_var0", "mont_adder_var0", "converter_var0",
                      "edwards_adder_var0", "t_bit0", "t_range_var0", "cond0_var", "doubler_var0", "cond_var0", "adder_var0", "step_stride",
                      "last_adder_var0")
EddsaPureLayout = namedtuple("EddsaPureLayout", PURE_LAYOUT_FIELDS)
EddsaPureLayout.__doc__ = """Where the segments of a witness row of eddsa_pure_circuit start (variable indices; variable 0 is ONE; a row has n_vars + 1 elements).
With W = ceil((508 + 8 msg_len) / 3) hash windows, S = ceil(W / 62) segments and a lone last window when W % 62 == 1:
    ax_var              A.x, A.y                                                 (public)
    msg_bit0            8 msg_len message bits, a byte's most significant first  (public)
    rx_var              R.x, R.y
    s_bit0              the 254 bits of s, least significant first
    pad_bit0            3 W - 508 - 8 msg_len (0, 1 or 2) padding bits, zero
    validator_var0, window_var0, fixed_adder_var0    as in EddsaLayout: 22, 127 x 2, 126 x 7
    rx_bit0, ax_bit0, t_bit0   254 bits, 253 results, 254 comparisons of field2bits_strict(R.x / A.x / the hash)
    rx_range_var0, ax_range_var0, t_range_var0       the 99 running products of BitsNotAbove(those bits, r - 1)
    hash_window_var0    W x (b0b1, the looked-up Montgomery y)                   stride 2
    mont_adder_var0     (W - S) x (lambda, X3, Y3): 61 to a full segment         stride 3
    converter_var0      S x (x, y) in the order of point_converters: the lone window's first
    edwards_adder_var0  (S - 1) x (beta, gamma, delta, epsilon, tau, x3, y3)     stride 7
    cond0_var, doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0     as in EddsaLayout"""


def pure_hash_windows(msg_len):
    """windows of the hash of bits(R.x) || bits(A.x) || 8 msg_len message bits, the last one zero-padded"""
    return (2 * FIELD_BITS + 8 * msg_len + 2) // 3


class _PureCore:
    """PureEdDSA over given variables: allocation and constraints in the reference's order, a BitsNotAbove behind each field2bits_strict"""

    def __init__(self, pb, B, ax, ay, rx, ry, s_bits, msg_bits):
        assert len(msg_bits) % 3 == (-2 * FIELD_BITS) % 3
        self.pb, self.ax, self.ay, self.rx, self.ry = pb, ax, ay, rx, ry
        mark = lambda: len(pb.values)
        at = self.at_var = {}
        at["validator_var0"] = mark()
        self.validator = PointValidator(pb, rx, ry)
        at["window_var0"] = mark()
        self.lhs = FixedBaseMul(pb, B, s_bits)
        at["fixed_adder_var0"] = self.lhs.adders[0].beta
        at["rx_bit0"] = mark()
        self.rx_bits = Field2BitsStrict(pb, rx)
        at["rx_range_var0"] = mark()
        self.rx_range = BitsNotAbove(pb, self.rx_bits.result(), FR - 1)
        at["ax_bit0"] = mark()
        self.ax_bits = Field2BitsStrict(pb, ax)
        at["ax_range_var0"] = mark()
        self.ax_range = BitsNotAbove(pb, self.ax_bits.result(), FR - 1)
        at["hash_window_var0"] = mark()
        self.hash = PedersenHashToBits(pb, EDDSA_SEED, self.rx_bits.result() + self.ax_bits.result() + list(msg_bits))
        fb = self.hash.hash.commitment
        at["mont_adder_var0"], at["converter_var0"] = fb.montgomery_adders[0].lam, fb.point_converters[0].x2
        at["edwards_adder_var0"] = fb.edward_adders[0].beta
        at["t_bit0"] = self.hash.tobits.bits[0]
        at["t_range_var0"] = mark()
        self.t_range = BitsNotAbove(pb, self.hash.result(), FR - 1)
        at["cond0_var"] = mark()
        self.at = sm = ScalarMult(pb, ax, ay, self.hash.result())
        at["last_adder_var0"] = mark()
        self.rhs = PointAdder(pb, rx, ry, sm.result_x(), sm.result_y())
        at.update(doubler_var0=sm.doublers[0].alpha, cond_var0=sm.conditionals[1].x2, adder_var0=sm.adders[0].beta,
                  step_stride=sm.doublers[1].alpha - sm.doublers[0].alpha)

    def generate_r1cs_constraints(self):
        pb = self.pb
        for g in (self.validator, self.lhs, self.rx_bits, self.rx_range, self.ax_bits, self.ax_range, self.hash, self.t_range, self.at, self.rhs):
            g.generate_r1cs_constraints()
        pb.add_r1cs_constraint(V(self.lhs.result_x()), 1, V(self.rhs.result_x()))
        pb.add_r1cs_constraint(V(self.lhs.result_y()), 1, V(self.rhs.result_y()))

    def generate_r1cs_witness(self, bits_value):
        self.validator.generate_r1cs_witness()
        self.lhs.generate_r1cs_witness()
        self.rx_bits.generate_r1cs_witness(bits_value.get("rx"))
        self.rx_range.generate_r1cs_witness()
        self.ax_bits.generate_r1cs_witness(bits_value.get("ax"))
        self.ax_range.generate_r1cs_witness()
        self.hash.generate_r1cs_witness(bits_value.get("t"))
        self.t_range.generate_r1cs_witness()
        self.at.generate_r1cs_witness()
        self.rhs.generate_r1cs_witness()

    def equation_holds(self):
        pb = self.pb
        return pb.val(self.lhs.result_x()) == pb.val(self.rhs.result_x()) and pb.val(self.lhs.result_y()) == pb.val(self.rhs.result_y())


def _bytes_to_bits(data):
    return [(byte >> (7 - k)) & 1 for byte in bytes(data) for k in range(8)]


class EddsaPureCircuit:
    """The gadgets of eddsa_pure_circuit on one protoboard; assign() writes another signature's witness into the same constraint system"""

    def __init__(self, msg_len=1, B=None):
        if int(msg_len) < 1:
            raise ValueError("msg_len is at least one byte")
        self.msg_len, self.B = int(msg_len), tuple(B) if B is not None else GENERATOR
        pb = self.pb = Protoboard()
        self.ax, self.ay = pb.allocate(), pb.allocate()
        self.msg_bits = pb.allocate_array(8 * self.msg_len)
        pb.set_input_sizes(2 + 8 * self.msg_len)
        self.rx, self.ry = pb.allocate(), pb.allocate()
        self.s_bits = pb.allocate_array(N_S_BITS)
        self.n_pad = 3 * pure_hash_windows(self.msg_len) - 2 * FIELD_BITS - 8 * self.msg_len
        pad0 = len(pb.values)
        self.pad_bits = pb.allocate_array(self.n_pad)
        self.core = _PureCore(pb, self.B, self.ax, self.ay, self.rx, self.ry, self.s_bits, self.msg_bits + self.pad_bits)
        self.layout = EddsaPureLayout(msg_len=self.msg_len, n_vars=len(pb.values) - 1, ax_var=self.ax, msg_bit0=self.msg_bits[0], rx_var=self.rx,
                                      s_bit0=self.s_bits[0], pad_bit0=pad0, **self.core.at_var)
        for b in self.s_bits + self.msg_bits:
            pb.add_r1cs_constraint(V(b), lc_add(1, lc_scale(V(b), -1)), 0)
        for b in self.pad_bits:
            pb.add_r1cs_constraint(V(b), 1, 0)
        self.core.generate_r1cs_constraints()
        self._r1cs = None

    def r1cs(self):
        if self._r1cs is None:
            self._r1cs = self.pb.to_r1cs()[0]
        return self._r1cs

    def assign(self, A, R, s, msg, bits_value=None):
        """generate_r1cs_witness for one signature; returns the witness (a list of n_vars + 1 ints).  s: an integer below 2^254; msg: msg_len
        bytes.  bits_value: {"rx" | "ax" | "t": an integer whose bits are written in the place of that element's own} (a test's non-canonical
        decomposition; everything downstream follows the bits written)"""
        pb, msg = self.pb, bytes(msg)
        assert 0 <= s < 1 << N_S_BITS and len(msg) == self.msg_len
        for var, v in zip([self.ax, self.ay, self.rx, self.ry], [A[0], A[1], R[0], R[1]]):
            pb.set_val(var, int(v))
        for var, b in zip(self.msg_bits, _bytes_to_bits(msg)):
            pb.set_val(var, b)
        for i, b in enumerate(self.s_bits):
            pb.set_val(b, (s >> i) & 1)
        for b in self.pad_bits:
            pb.set_val(b, 0)
        self.core.generate_r1cs_witness(bits_value or {})
        return list(pb.values)

    def public_inputs(self, A, msg):
        return [int(A[0]) % FR, int(A[1]) % FR] + _bytes_to_bits(msg)

    def equation_holds(self):
        """the two closing constraints alone: lhs == rhs"""
        return self.core.equation_holds()


def eddsa_pure_circuit(msg_len=1, B=None, A=None, R=None, s=None, msg=None):
    """PureEdDSA verification (src/jubjub/eddsa.cpp), S B == R + t A with t = the x of pedersen_hash_bits("EdDSA_Verify.RAM", bits(R.x) || bits(A.x) || M):

        1. PointValidator(R)                          2. lhs = FixedBaseMul(B, bits of s), 254 bits
        3. Field2BitsStrict(R.x), Field2BitsStrict(A.x)   4. PedersenHashToBits over those bits and the message bits
        5. At = ScalarMult(A, bits of t)              6. rhs = PointAdder(R, At)        7. lhs.x == rhs.x, lhs.y == rhs.y

    PUBLIC: A.x, A.y and the 8 msg_len message bits (a byte's most significant bit first).  PRIVATE: R, the bits of s, everything derived.
    Added to the reference: booleanity of every bit of s and of the message; BitsNotAbove(bits, r - 1) behind each of the three
    field2bits_strict (the gadget alone pins only a congruent value); and, when 508 + 8 msg_len is no multiple of 3, one or two private
    padding bits constrained to zero -- the zero-extended last window of pedersen_hash_bits -- so every msg_len has a circuit that agrees with
    EdDSAVerifier("pure").  Returns (protoboard, EddsaPureLayout); with A, R, s and msg given the protoboard holds that signature's witness."""
    c = EddsaPureCircuit(msg_len, B)
    if A is not None:
        c.assign(A, R, s, msg)
    return c.pb, c.layout


HASH_LAYOUT_FIELDS = tuple(f for f in PURE_LAYOUT_FIELDS if f != "pad_bit0") + (
    "m_pad_bit0", "m_window_var0", "m_mont_adder_var0", "m_converter_var0", "m_edwards_adder_var0", "m_bit0", "m_range_var0")
EddsaHashLayout = namedtuple("EddsaHashLayout", HASH_LAYOUT_FIELDS)
EddsaHashLayout.__doc__ = """Where the segments of a witness row of EddsaHashCircuit start (variable indices; variable 0 is ONE; a row has n_vars + 1 elements).
Every field of EddsaPureLayout but pad_bit0, with the same meaning: the hash "EdDSA_Verify.RAM" covers bits(R.x) || bits(A.x) || bits(M.x), 762
bits, so W = 254 windows in S = 5 segments of 62, 62, 62, 62 and 6, no padding bit and no lone window.  For the message hash "EdDSA_Verify.M", with
W_m = ceil(8 msg_len / 3) windows and S_m = ceil(W_m / 62) segments (a lone last window when W_m % 62 == 1):
    m_pad_bit0            (-8 msg_len) mod 3 padding bits, zero                  (none when msg_len is a multiple of 3)
    m_window_var0         W_m x (b0b1, the looked-up Montgomery y)               stride 2
    m_mont_adder_var0     (W_m - S_m) x (lambda, X3, Y3)                         stride 3
    m_converter_var0      S_m x (x, y) in the order of point_converters: the lone window's first
    m_edwards_adder_var0  (S_m - 1) x 7                                          (none when W_m <= 62, msg_len <= 23)
    m_bit0                254 bits, 253 results, 254 comparisons of field2bits_strict(M.x): the bits are the third part of the RAM hash's input
    m_range_var0          the 99 running products of BitsNotAbove(those bits, r - 1)
An empty segment's field holds the variable the segment would start at."""


def hash_msg_windows(msg_len):
    """windows of the message hash of EddsaHashCircuit: 8 msg_len bits, the last window zero-padded"""
    return (8 * msg_len + 2) // 3


class EddsaHashCircuit:
    """The reference's EdDSA: M = PedersenHashToBits("EdDSA_Verify.M", the message bits) and PureEdDSA over the 254 bits of M.  Public inputs and
    additions as eddsa_pure_circuit, a BitsNotAbove behind the fourth decomposition too, zero padding bits for the message hash when 8 msg_len
    is no multiple of 3.  .layout (an EddsaHashLayout) is the row that k_eddsa_fill_hash fills on the device"""

    def __init__(self, msg_len=1, B=None):
        if int(msg_len) < 1:
            raise ValueError("msg_len is at least one byte")
        self.msg_len, self.B = int(msg_len), tuple(B) if B is not None else GENERATOR
        pb = self.pb = Protoboard()
        self.ax, self.ay = pb.allocate(), pb.allocate()
        self.msg_bits = pb.allocate_array(8 * self.msg_len)
        pb.set_input_sizes(2 + 8 * self.msg_len)
        self.rx, self.ry = pb.allocate(), pb.allocate()
        self.s_bits = pb.allocate_array(N_S_BITS)
        mark = lambda: len(pb.values)
        at = {"m_pad_bit0": mark()}
        self.pad_bits = pb.allocate_array((-8 * self.msg_len) % 3)
        at["m_window_var0"] = mark()
        self.msg_hashed = PedersenHashToBits(pb, PEDERSEN_MSG_SEED, self.msg_bits + self.pad_bits)
        fb = self.msg_hashed.hash.commitment
        at["m_bit0"] = self.msg_hashed.tobits.bits[0]
        at["m_mont_adder_var0"], at["m_converter_var0"] = fb.montgomery_adders[0].lam, fb.point_converters[0].x2
        at["m_edwards_adder_var0"] = fb.edward_adders[0].beta if fb.edward_adders else at["m_bit0"]
        at["m_range_var0"] = mark()
        self.msg_range = BitsNotAbove(pb, self.msg_hashed.result(), FR - 1)
        self.core = _PureCore(pb, self.B, self.ax, self.ay, self.rx, self.ry, self.s_bits, self.msg_hashed.result())
        self.layout = EddsaHashLayout(msg_len=self.msg_len, n_vars=len(pb.values) - 1, ax_var=self.ax, msg_bit0=self.msg_bits[0], rx_var=self.rx,
                                      s_bit0=self.s_bits[0], **at, **self.core.at_var)
        for b in self.s_bits + self.msg_bits:
            pb.add_r1cs_constraint(V(b), lc_add(1, lc_scale(V(b), -1)), 0)
        for b in self.pad_bits:
            pb.add_r1cs_constraint(V(b), 1, 0)
        self.msg_hashed.generate_r1cs_constraints()
        self.msg_range.generate_r1cs_constraints()
        self.core.generate_r1cs_constraints()
        self._r1cs = None

    r1cs = EddsaPureCircuit.r1cs
    public_inputs = EddsaPureCircuit.public_inputs

    def assign(self, A, R, s, msg, bits_value=None):
        pb, msg = self.pb, bytes(msg)
        assert 0 <= s < 1 << N_S_BITS and len(msg) == self.msg_len
        for var, v in zip([self.ax, self.ay, self.rx, self.ry], [A[0], A[1], R[0], R[1]]):
            pb.set_val(var, int(v))
        for var, b in zip(self.msg_bits, _bytes_to_bits(msg)):
            pb.set_val(var, b)
        for i, b in enumerate(self.s_bits):
            pb.set_val(b, (s >> i) & 1)
        for b in self.pad_bits:
            pb.set_val(b, 0)
        self.msg_hashed.generate_r1cs_witness((bits_value or {}).get("m"))
        self.msg_range.generate_r1cs_witness()
        self.core.generate_r1cs_witness(bits_value or {})
        return list(pb.values)

    def equation_holds(self):
        return self.core.equation_holds()


def eddsa_hash_circuit(msg_len=1, B=None):
    """(protoboard, EddsaHashLayout) of EddsaHashCircuit: the reference's EdDSA, M hashed with the Pedersen hash before PureEdDSA"""
    c = EddsaHashCircuit(msg_len, B)
    return c.pb, c.layout
