"""The in-circuit Baby JubJub gadgets (ethsnarks_amd/jubjub_gadgets.py) on the host: every gadget satisfied, equal to the expected values of the
reference's own gadget tests (tests/golden/jubjub_gadget_kats.json) and to the integer restatement of jubjub_cases.py on the directed points and
scalars, unsatisfied after one flipped witness value, and of the variable and constraint counts the reference's constructors imply.  Then the
composed MiMC-EdDSA circuit against jubjub_cases.sign / verify.  No device, no library."""
import json
import os
import random

import pytest

from ethsnarks_amd import gadgets as G, jubjub_gadgets as JG
from ethsnarks_amd.fields import FR
import jubjub_cases as JC

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jubjub_gadget_kats.json")) as _f:
    KATS = json.load(_f)


def pt(v):
    return (int(v[0]), int(v[1]))


def board(*values):
    pb = G.Protoboard()
    return pb, [pb.allocate(v) for v in values]


def run(g):
    g.generate_r1cs_witness()
    g.generate_r1cs_constraints()
    return g


def counts(pb, n_inputs):
    """(variables the gadget allocated, constraints)"""
    return len(pb.values) - 1 - n_inputs, pb.num_constraints()


def every_flip_breaks(pb, first_var):
    """one witness value of the gadget changed at a time: never satisfied"""
    assert pb.is_satisfied()
    for var in range(first_var, len(pb.values)):
        old = pb.val(var)
        pb.set_val(var, old + 1)
        assert not pb.is_satisfied(), var
        pb.set_val(var, old)
    assert pb.is_satisfied()


def bits_of(v, n):
    return [(v >> i) & 1 for i in range(n)]


# ---------------------------------------------------------------- lookups
def test_lookup_1bit():
    """test_lookup_1bit.cpp: two random constants, both indices; 1 variable, 1 constraint"""
    rng = random.Random(1)
    c = [rng.randrange(FR), rng.randrange(FR)]
    for i in (0, 1):
        pb, (b,) = board(i)
        g = run(JG.Lookup1bit(pb, c, b))
        assert pb.val(g.result()) == c[i] and counts(pb, 1) == (1, 1)
        every_flip_breaks(pb, g.result())


def test_lookup_2bit():
    """test_lookup_2bit.cpp: four random constants, the four indices (bit 0 the low one); 1 variable, 1 constraint"""
    rng = random.Random(2)
    c = [rng.randrange(FR) for _ in range(4)]
    for i in range(4):
        pb, bits = board(i & 1, i >> 1)
        g = run(JG.Lookup2bit(pb, c, bits))
        assert pb.val(g.result()) == c[i] and counts(pb, 2) == (1, 1)
        every_flip_breaks(pb, g.result())


# ---------------------------------------------------------------- the point gadgets
ADD_PAIRS = [(JC.GENERATOR, JC.POINT_A), (JC.POINT_A, JC.POINT_A), (JC.IDENTITY, JC.IDENTITY), (JC.IDENTITY, JC.GENERATOR), (JC.GENERATOR, JC.neg(JC.GENERATOR))]
ADD_PAIRS += [(p, p) for p in JC.LOW_ORDER] + [(p, JC.GENERATOR) for p in JC.LOW_ORDER] + [(JC.LOW_ORDER[3], JC.LOW_ORDER[5])]


def test_point_adder():
    """test_jubjub_add.cpp; the eight low-order points, the identity and P + P through the same constraints; 7 variables, 7 constraints"""
    k = KATS["add"]
    for p, q, want in [(pt(k["a"]), pt(k["b"]), pt(k["sum"]))] + [(p, q, JC.add(p, q)) for p, q in ADD_PAIRS]:
        pb, v = board(p[0], p[1], q[0], q[1])
        g = run(JG.PointAdder(pb, *v))
        assert (pb.val(g.result_x()), pb.val(g.result_y())) == want == JC.affine_add_reference(p, q), (p, q)
        assert pb.is_satisfied() and counts(pb, 4) == (7, 7)
    every_flip_breaks(pb, g.beta)


def test_point_doubler():
    """test_jubjub_dbl.cpp; every directed point; 6 variables, 6 constraints"""
    k = KATS["dbl"]
    for p, want in [(pt(k["a"]), pt(k["double"]))] + [(p, JC.double(p)) for p in JC.POINTS]:
        pb, v = board(*p)
        g = run(JG.PointDoubler(pb, *v))
        assert (pb.val(g.result_x()), pb.val(g.result_y())) == want == JC.add(p, p), p
        assert pb.is_satisfied() and counts(pb, 2) == (6, 6)
    every_flip_breaks(pb, g.alpha)


def test_conditional_point():
    """2 variables, 2 constraints; bit 0 gives the identity"""
    for p in (JC.GENERATOR, JC.IDENTITY, JC.LOW_ORDER[3]):
        for bit in (0, 1):
            pb, v = board(p[0], p[1], bit)
            g = run(JG.ConditionalPoint(pb, *v))
            assert (pb.val(g.result_x()), pb.val(g.result_y())) == (p if bit else JC.IDENTITY)
            assert counts(pb, 3) == (2, 2)
            every_flip_breaks(pb, g.x2)


def test_is_on_curve():
    """test_jubjub_isoncurve.cpp; 2 variables, 3 constraints"""
    for p, want in [(pt(p), w) for p, w in KATS["on_curve"]] + [(p, True) for p in JC.POINTS] + [(JC.OFF_CURVE, False)]:
        pb, v = board(*p)
        run(JG.IsOnCurve(pb, *v))
        assert pb.is_satisfied() == want == JC.on_curve(p), p
        assert counts(pb, 2) == (2, 3)
    pb, v = board(*JC.GENERATOR)
    g = run(JG.IsOnCurve(pb, *v))
    every_flip_breaks(pb, g.xx)


def test_not_low_order_and_validator():
    """test_jubjub_notloworder.cpp: the eight low-order points are refused, three others pass.  NotLowOrder: 3 x 6 + 2 variables, 3 x 6 + 3 + 1
    constraints; PointValidator adds IsOnCurve: 22 variables, 25 constraints"""
    low = [pt(p) for p in KATS["low_order"]]
    assert sorted(low) == sorted(JC.LOW_ORDER)
    for p, want in [(p, False) for p in low] + [(pt(p), True) for p in KATS["not_low_order"]] + [(JC.GENERATOR, True)]:
        pb, v = board(*p)
        g = run(JG.NotLowOrder(pb, *v))
        assert pb.is_satisfied() == want, p
        assert (pb.val(g.doublers[-1].result_x()), pb.val(g.doublers[-1].result_y())) == JC.mul(p, 8)
        assert counts(pb, 2) == (20, 22)
        pb, v = board(*p)
        run(JG.PointValidator(pb, *v))
        assert pb.is_satisfied() == want and counts(pb, 2) == (22, 25)
    pb, v = board(*JC.OFF_CURVE)
    run(JG.PointValidator(pb, *v))
    assert not pb.is_satisfied()
    pb, v = board(*JC.GENERATOR)
    g = run(JG.PointValidator(pb, *v))
    every_flip_breaks(pb, g.notloworder.doublers[0].alpha)


SCALARS = [0, 1, JC.L, (1 << 100) - 1, (1 << 253) - 1, (1 << 254) - 1, JC.Q - 1, 0x2AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA]
assert all(0 <= k < 1 << 254 for k in SCALARS)


def test_scalar_mult():
    """test_jubjub_mul.cpp (252 bits); 254 bits: scalars 0, 1, L, 2^k - 1 and all-ones on the generator, a few on low-order points.
    n bits: 2 + 15 (n - 1) variables, 6 (n - 1) + 2 n + 7 (n - 1) constraints"""
    k = KATS["mul"]
    cases = [(pt(k["base"]), int(k["scalar"]), k["bits"], pt(k["product"]))]
    cases += [(JC.GENERATOR, s, 254, JC.mul(JC.GENERATOR, s)) for s in SCALARS]
    cases += [(p, s, 254, JC.mul(p, s)) for p in (JC.IDENTITY, JC.LOW_ORDER[1], JC.LOW_ORDER[3]) for s in (0, 7, (1 << 254) - 1)]
    for p, s, n, want in cases:
        pb, v = board(*(list(p) + bits_of(s, n)))
        g = run(JG.ScalarMult(pb, v[0], v[1], v[2:]))
        assert (pb.val(g.result_x()), pb.val(g.result_y())) == want, (p, s)
        assert pb.is_satisfied() and counts(pb, 2 + n) == (2 + 15 * (n - 1), 15 * (n - 1) + 2)
    pb, v = board(*(list(JC.POINT_A) + bits_of(0b1011, 4)))
    g = run(JG.ScalarMult(pb, v[0], v[1], v[2:]))
    every_flip_breaks(pb, g.conditionals[0].x2)


def test_fixed_base_mul():
    """test_jubjub_mul_fixed.cpp (252 bits); 254 bits on the generator.  n bits, w = n / 2 windows: 2 w + 7 (w - 1) variables and as many
    constraints; window i of the table is [identity, P, 2 P, 3 P] with P = 4^i B"""
    k = KATS["mul"]
    cases = [(pt(k["base"]), int(k["scalar"]), k["bits"], pt(k["product"]))]
    cases += [(JC.GENERATOR, s, 254, JC.mul(JC.GENERATOR, s)) for s in SCALARS] + [(JC.LOW_ORDER[3], (1 << 254) - 1, 254, JC.mul(JC.LOW_ORDER[3], (1 << 254) - 1))]
    for p, s, n, want in cases:
        pb, v = board(*bits_of(s, n))
        g = run(JG.FixedBaseMul(pb, p, v))
        w = n // 2
        assert (pb.val(g.result_x()), pb.val(g.result_y())) == want, (p, s)
        assert pb.is_satisfied() and counts(pb, n) == (2 * w + 7 * (w - 1), 2 * w + 7 * (w - 1))
    table = JG.fixed_base_table(JC.GENERATOR, 127)
    for i in (0, 1, 63, 126):
        assert table[i] == [JC.IDENTITY] + [JC.mul(JC.GENERATOR, m << (2 * i)) for m in (1, 2, 3)]
    pb, v = board(*bits_of(0b100111, 6))
    g = run(JG.FixedBaseMul(pb, JC.GENERATOR, v))
    every_flip_breaks(pb, g.windows_x[0].r)


def test_field2bits_strict_and_range_check():
    """test_field2bits.cpp: 0, 1 and r - 1 are satisfied.  254 + 253 + 254 variables; 1 + 254 + 254 + 253 constraints.  The reference's gadget
    alone accepts the bits of v + r; BitsNotAbove(bits, r - 1) -- 99 variables, 253 constraints -- refuses them and accepts every v < r"""
    for text, want in KATS["field2bits"]:
        pb, (x,) = board(int(text))
        g = run(JG.Field2BitsStrict(pb, x))
        assert pb.is_satisfied() == want and [pb.val(b) for b in g.result()] == bits_of(int(text), 254)
        assert counts(pb, 1) == (761, 762)
    rng = random.Random(3)
    for v in [0, 1, FR - 1, (1 << 254) - FR - 1, (1 << 253) - 1, 1 << 253] + [rng.randrange(FR) for _ in range(4)]:
        for alias in (False, True):
            if alias and v + FR >= 1 << 254:
                continue
            pb, (x,) = board(v)
            g = JG.Field2BitsStrict(pb, x)
            g.generate_r1cs_witness(v + FR if alias else None)
            g.generate_r1cs_constraints()
            assert pb.is_satisfied()                                   # congruent is all the reference's gadget asks
            before = len(pb.values), pb.num_constraints()
            rc = JG.BitsNotAbove(pb, g.result(), FR - 1)
            run(rc)
            assert (len(pb.values) - before[0], pb.num_constraints() - before[1]) == (99, 253) and rc.n_vars() == 99
            assert pb.is_satisfied() == (not alias), (v, alias)
    pb, (x,) = board(rng.randrange(FR))
    g = run(JG.Field2BitsStrict(pb, x))
    rc = run(JG.BitsNotAbove(pb, g.result(), FR - 1))
    every_flip_breaks(pb, g.bits[0])


def test_mimc_constants_argument_leaves_existing_circuits_alone():
    r1, w1, d1 = G.mimc_preimage_circuit(2)
    assert d1 == G.mimc_hash(w1[3:5], 0)
    pb = G.Protoboard()
    iv, m = pb.allocate(0), pb.allocate_array(3, [5, 6, 7])
    g = run(G.MiMCe7HashGadget(pb, iv, m, constants=G.mimc_constants(seed=JC.RAM)))
    assert pb.is_satisfied() and pb.val(g.result()) == JC.mimc_hash_ram([5, 6, 7]) != G.mimc_hash([5, 6, 7], 0)


# ---------------------------------------------------------------- the composed circuit
@pytest.fixture(scope="module")
def circuit():
    return JG.EddsaMimcCircuit(1)


def signed(seed, length=1, alias=None):
    """a signature; alias=True: one whose t + r still fits 254 bits"""
    rng = random.Random(seed)
    while True:
        A, (R, s), msg = JC.sign("mimc", JC.make_msg("mimc", length, rng), rng.randrange(1, JC.L))
        t = JC.hash_public("mimc", R, A, msg)
        if s < 1 << 254 and (alias is None or (t + FR < 1 << 254) == alias):
            return A, R, s, msg, t


def test_circuit_shape(circuit):
    """2 + m public inputs; variables and constraints as the sum of the parts (m = 1: 7 907 and 8 062)"""
    pb, lay = JG.eddsa_mimc_circuit(1)
    m = 1
    n_vars = (2 + m + 2 + 254 + 1) + 22 + (254 + 7 * 126) + (4 + m) * 365 + 761 + 99 + (2 + 15 * 253) + 7
    n_cons = 254 + 1 + 25 + (254 + 7 * 126) + (4 + m) * 365 + 762 + 253 + (15 * 253 + 2) + 7 + 2
    assert (lay.n_vars, pb.num_constraints(), pb.n_inputs) == (n_vars, n_cons, 3) == (7907, 8062, 3)
    assert lay == circuit.layout and lay.step_stride == 15 and (lay.cond_var0, lay.adder_var0) == (lay.doubler_var0 + 6, lay.doubler_var0 + 8)
    assert lay.last_adder_var0 + 7 == lay.n_vars + 1 and lay.cond0_var + 2 == lay.doubler_var0
    # every offset, as tests/cpp/eddsa_fill_sanity.cpp layout1() restates them: a change of the row shows here and names the file to follow
    assert tuple(lay) == (1, 7907, 1, 3, 4, 6, 260, 261, 283, 537, 1419, 3244, 4005, 4104, 4106, 4112, 4114, 15, 7901)
    pb3, lay3 = JG.eddsa_mimc_circuit(3)
    assert lay3.n_vars == n_vars + 2 * 366 and pb3.n_inputs == 5


def test_circuit_accepts_signatures(circuit):
    for seed in (1, 2):
        A, R, s, msg, t = signed(seed)
        w = circuit.assign(A, R, s, msg)
        assert circuit.pb.is_satisfied() and circuit.equation_holds() and JC.verify("mimc", A, (R, s), msg)
        assert w[1:4] == circuit.public_inputs(A, msg) and circuit.pb.val(circuit.hash.result()) == t
        assert circuit.r1cs().is_satisfied(w) if seed == 1 else True
    A, R, s, msg, _ = signed(5, 3)
    pb, _ = JG.eddsa_mimc_circuit(3, A=A, R=R, s=s, msg=msg)
    assert pb.is_satisfied()
    B = JC.mul(JC.GENERATOR, 77)                                       # another base point
    A, (R, s), msg = JC.sign("mimc", [9], 1234567, B)
    pb, _ = JG.eddsa_mimc_circuit(1, B=B, A=A, R=R, s=s % (1 << 254), msg=msg)
    assert pb.is_satisfied() == (s < 1 << 254)


def test_circuit_refuses_wrong_signatures(circuit):
    A, R, s, msg, t = signed(11, alias=True)
    other = signed(12)
    bad = {"flipped message": (A, R, s, JC.flip_first("mimc", msg)), "flipped s": (A, R, s ^ 1, msg), "swapped R": (A, other[1], s, msg),
           "swapped A": (other[0], R, s, msg)}
    for label, (a, r, s_, m) in bad.items():
        circuit.assign(a, r, s_, m)
        assert not circuit.pb.is_satisfied() and not circuit.equation_holds() and not JC.verify("mimc", a, (r, s_), m), label
    circuit.assign(A, R, s, msg, t_bits_value=t + FR)                  # the other decomposition of t: congruent, and t A is not (t + r) A
    assert not circuit.pb.is_satisfied()
    circuit.assign(A, R, s, msg)
    assert circuit.pb.is_satisfied()


def test_circuit_is_stricter_on_low_order_r(circuit):
    """the verifier accepts A = R = identity with s = 0; PointValidator(R) does not: the row is complete, lhs == rhs holds, NotLowOrder fails"""
    assert JC.verify("mimc", JC.IDENTITY, (JC.IDENTITY, 0), [7])
    circuit.assign(JC.IDENTITY, JC.IDENTITY, 0, [7])
    assert circuit.equation_holds() and not circuit.pb.is_satisfied()
