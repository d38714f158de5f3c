"""The in-circuit Pedersen hash on the CPU (ethsnarks_amd/jubjub_gadgets.py): lookup_signed_3bit, the Montgomery adder and converter,
fixed_base_mul_zcash, PedersenHash / PedersenHashToBits and the PureEdDSA / EdDSA circuits composed of them, against the expected values of the
reference's own gadget tests (tests/golden/pedersen_gadget_kats.json) and the integer restatement of jubjub_cases.py.  Every protoboard is
checked satisfied by its generated witness and unsatisfied after one flipped bit."""
import random

import pytest

from ethsnarks_amd import jubjub_gadgets as JG
from ethsnarks_amd.fields import FR
from ethsnarks_amd.gadgets import Protoboard, V
import eddsa_pure_cases as PC
import jubjub_cases as JC

KATS = PC.KATS


def hash_board(name, bits, cls=JG.PedersenHash):
    pb = Protoboard()
    var = pb.allocate_array(len(bits), [int(b) for b in bits])
    g = cls(pb, name, var)
    g.generate_r1cs_constraints()
    g.generate_r1cs_witness()
    return pb, var, g


def flipped_fails(pb, var):
    pb.set_val(var, 1 - pb.val(var))
    bad = not pb.is_satisfied()
    pb.set_val(var, 1 - pb.val(var))
    return bad and pb.is_satisfied()


def field_bits(v, n):
    return [(v >> i) & 1 for i in range(n)]


def implied_counts(n_windows):
    """(variables, constraints) of fixed_base_mul_zcash: 2 + 2 a window, 3 + 3 a Montgomery adder, 2 + 2 a converter, 7 + 7 an Edwards adder"""
    seg = -(-n_windows // 62)
    n = 2 * n_windows + 3 * (n_windows - seg) + 2 * seg + 7 * (seg - 1)
    return n, n


# ---------------------------------------------------------------- the small gadgets
def test_basepoints_are_those_of_the_restatement():
    for name, i in ((b"test", 0), (b"EdDSA_Verify.RAM", 2), (b"EdDSA_Verify.M", 0), (b"x" * 28, 0xFFFF)):
        p = JG.pedersen_basepoint(name, i)
        assert p == JC.basepoint(name, i) and JC.on_curve(p) and JC.mul(p, JC.L) == JC.IDENTITY
    with pytest.raises(ValueError):
        JG.pedersen_basepoint(b"x" * 29, 0)
    with pytest.raises(ValueError):
        JG.pedersen_basepoint(b"x", 0x10000)


def test_lookup_signed_3bit():
    c = [11, FR - 5, 123456789, 3]
    for digit in range(8):
        pb = Protoboard()
        bits = pb.allocate_array(3, field_bits(digit, 3))
        g = JG.LookupSigned3bit(pb, c, bits)
        assert (g.b0b1, g.r) == (4, 5)                                 # b0b1 is allocated before r
        g.generate_r1cs_constraints()
        g.generate_r1cs_witness()
        assert pb.num_constraints() == 2 and pb.is_satisfied()
        assert pb.val(g.result()) == (-c[digit & 3] if digit > 3 else c[digit & 3]) % FR and pb.val(g.b0b1) == (digit & 3 == 3)
        assert sum(k * pb.val(i) for i, k in g.lc(c).items()) % FR == c[digit & 3]
        assert all(flipped_fails(pb, b) for b in bits)


def test_montgomery_adder_and_converter():
    rng = random.Random(3)
    for _ in range(4):
        p, q = JC.mul(JC.GENERATOR, rng.randrange(1, JC.L)), JC.mul(JC.GENERATOR, rng.randrange(1, JC.L))
        (u1, v1), (u2, v2) = JG.as_montgomery(p), JG.as_montgomery(q)
        pb = Protoboard()
        y1, y2, x2 = pb.allocate(v1), pb.allocate(v2), pb.allocate(u2)
        add = JG.MontgomeryAdder(pb, u1, y1, V(x2), y2)                # a constant and a variable as the linear combinations
        assert (add.lam, add.x3, add.y3) == (4, 5, 6)
        conv = JG.MontgomeryToEdwards(pb, V(add.result_x()), add.result_y())
        for g in (add, conv):
            g.generate_r1cs_constraints()
            g.generate_r1cs_witness()
        assert pb.num_constraints() == 5 and pb.is_satisfied()
        assert (pb.val(add.x3), pb.val(add.y3)) == JG.as_montgomery(JC.add(p, q))
        assert (pb.val(conv.result_x()), pb.val(conv.result_y())) == JC.add(p, q)
        pb.set_val(add.lam, pb.val(add.lam) + 1)
        assert not pb.is_satisfied()


# ---------------------------------------------------------------- the reference's vectors
@pytest.mark.parametrize("case", KATS["hash_bytes"], ids=lambda c: c["data"][:6])
def test_reference_hash_of_bytes(case):
    bits = JC.bytes_to_bits(case["data"].encode("ascii"))
    pb, var, g = hash_board(case["name"], bits)
    want = (int(case["x"]), int(case["y"]))
    assert (pb.val(g.result_x()), pb.val(g.result_y())) == want == JC.pedersen_bits(case["name"], bits)
    assert pb.is_satisfied() and flipped_fails(pb, var[0]) and flipped_fails(pb, var[-1])


@pytest.mark.parametrize("case", KATS["hash_bits"], ids=lambda c: str(len(c["bits"])))
def test_reference_hash_of_bits(case):
    pb, var, g = hash_board(case["name"], case["bits"])
    want = (int(case["x"]), int(case["y"]))
    assert (pb.val(g.result_x()), pb.val(g.result_y())) == want == JC.pedersen_bits(case["name"], case["bits"])
    assert pb.is_satisfied() and flipped_fails(pb, var[len(var) // 2])
    assert (len(pb.values) - 1 - len(var), pb.num_constraints()) == implied_counts(len(var) // 3)


def test_reference_fixed_base_mul_zcash():
    k = KATS["mul_fixed_zcash"]
    rows = [(field_bits(int(c["scalar"]), c["n_bits"]), c) for c in k["scalars"]] + [([int(b) for b in c["bits"]], c) for c in k["bits"]]
    rows += [(JC.bytes_to_bits(c["data"].encode("ascii")), c) for c in k["bytes"]]
    for bits, c in rows:
        pb, var, g = hash_board(k["name"], bits)
        assert (pb.val(g.result_x()), pb.val(g.result_y())) == (int(c["x"]), int(c["y"])) == JC.pedersen_bits(k["name"], bits)
        assert pb.is_satisfied() and flipped_fails(pb, var[2])


# ---------------------------------------------------------------- segment boundaries
@pytest.mark.parametrize("n_windows", [2, 61, 62, 63, 124, 125, 187])
def test_window_counts(n_windows):
    """one segment, a full one, the lone-window branch (63, 125, 187), two full ones: value, counts, and the place of the lone converter"""
    rng = random.Random(n_windows)
    bits = [rng.randrange(2) for _ in range(3 * n_windows)]
    pb, var, g = hash_board(b"test", bits)
    fb = g.commitment
    assert (pb.val(g.result_x()), pb.val(g.result_y())) == JC.pedersen_bits(b"test", bits)
    assert pb.is_satisfied() and flipped_fails(pb, var[0]) and flipped_fails(pb, var[-1])
    assert (len(pb.values) - 1 - len(var), pb.num_constraints()) == implied_counts(n_windows)
    seg = -(-n_windows // 62)
    assert (len(fb.windows_y), len(fb.montgomery_adders), len(fb.point_converters), len(fb.edward_adders)) == (n_windows, n_windows - seg, seg, seg - 1)
    first = fb.point_converters[0]
    if n_windows % 62 == 1:                                            # the lone window's converter stands FIRST and follows the adders in allocation
        assert first.y1 == fb.windows_y[-1].result() and first.x2 == fb.montgomery_adders[-1].y3 + 1
        assert (pb.val(first.x2), pb.val(first.y2)) == JC.affine(JC.eneg(JC.table_row(b"test", n_windows - 1)[bits[-3] + 2 * bits[-2]])
                                                                 if bits[-1] else JC.table_row(b"test", n_windows - 1)[bits[-3] + 2 * bits[-2]])
    else:
        assert first.y1 == fb.montgomery_adders[min(n_windows, 62) - 2].result_y()
    assert fb.windows_y[0].b0b1 == len(var) + 1 and fb.montgomery_adders[0].lam == len(var) + 2 * n_windows + 1


@pytest.mark.parametrize("bits", [[1] * 189, [0] * 189, [0, 0, 1] * 63, [1, 1, 0] * 63], ids=["ones", "zeros", "sign only", "digit 4"])
def test_constant_windows(bits):
    """the sign bit set in every window, all-zero bits, the largest digit: no adder meets equal x, no converter a zero denominator"""
    pb, var, g = hash_board(b"EdDSA_Verify.RAM", bits)
    assert (pb.val(g.result_x()), pb.val(g.result_y())) == JC.pedersen_bits(b"EdDSA_Verify.RAM", bits) and pb.is_satisfied()
    fb = g.commitment
    assert all(pb.val(a.lam) for a in fb.montgomery_adders) and all(pb.val(c.x2) for c in fb.point_converters)


def test_refused_bit_counts():
    for n in (3, 4, 0, 7):                                             # one window (the reference reads an empty vector), no multiple of 3
        pb = Protoboard()
        with pytest.raises(ValueError):
            JG.PedersenHash(pb, b"test", pb.allocate_array(n))
    pb = Protoboard()
    with pytest.raises(ValueError):
        JG.FixedBaseMulZcash(pb, [JC.basepoint(b"test", 0)], pb.allocate_array(3 * 63))   # two base points needed


def test_hash_to_bits():
    bits = [1, 0, 1] * 70
    pb, var, g = hash_board(b"EdDSA_Verify.M", bits, JG.PedersenHashToBits)
    x = JC.pedersen_bits(b"EdDSA_Verify.M", bits)[0]
    assert [pb.val(b) for b in g.result()] == JC.field_bits(x) and pb.is_satisfied()
    assert len(pb.values) - 1 - len(var) == implied_counts(70)[0] + 3 * 254 - 1


# ---------------------------------------------------------------- the circuits
_CIRCUITS = {}


def pure(msg_len):
    if msg_len not in _CIRCUITS:
        _CIRCUITS[msg_len] = JG.EddsaPureCircuit(msg_len)
    return _CIRCUITS[msg_len]


def test_reference_signatures_satisfy_both_circuits():
    e = KATS["eddsa"]
    A = tuple(int(v) for v in e["A"])
    c = pure(4)
    sig = e["pure"]
    w = c.assign(A, tuple(int(v) for v in sig["R"]), int(sig["s"]), sig["msg"].encode("ascii"))
    assert c.pb.is_satisfied() and c.r1cs().is_satisfied(w) and c.equation_holds() and c.n_pad == 0
    assert w[1:1 + c.pb.n_inputs] == c.public_inputs(A, b"abcd")
    assert flipped_fails(c.pb, c.msg_bits[5]) and flipped_fails(c.pb, c.s_bits[7])
    h = JG.EddsaHashCircuit(3)
    sig = e["hash"]
    h.assign(A, tuple(int(v) for v in sig["R"]), int(sig["s"]), sig["msg"].encode("ascii"))
    assert h.pb.is_satisfied() and h.equation_holds() and len(h.pad_bits) == 0
    assert [h.pb.val(b) for b in h.msg_hashed.result()] == JC.field_bits(JC.pedersen_bytes(JC.MSG, b"abc")[0])
    assert flipped_fails(h.pb, h.msg_bits[23])
    h.assign(A, tuple(int(v) for v in sig["R"]), int(sig["s"]), b"abd")
    assert not h.pb.is_satisfied()


@pytest.mark.parametrize("msg_len", [1, 4])
def test_circuit_counts(msg_len):
    """the counts the constructors imply (DESIGN 5k quotes them): 8 679 / 9 145 at one byte, 8 743 / 9 209 at four, a domain of 2^14"""
    c = pure(msg_len)
    W = JG.pure_hash_windows(msg_len)
    pad = 3 * W - 508 - 8 * msg_len
    hv, hc = implied_counts(W)
    strict_v, strict_c, range_v, range_c = 3 * 254 - 1, 1 + 254 + 254 + 253, 99, 253
    n_vars = 2 + 8 * msg_len + 2 + 254 + pad + 22 + 127 * 2 + 126 * 7 + 3 * (strict_v + range_v) + hv + 2 + 253 * 15 + 7
    n_cons = 254 + 8 * msg_len + pad + 25 + 127 * 2 + 126 * 7 + 3 * (strict_c + range_c) + hc + 253 * 6 + 254 * 2 + 253 * 7 + 7 + 2
    r = c.r1cs()
    assert (r.V, r.nC, r.nIn) == (n_vars, n_cons, 2 + 8 * msg_len) == (c.layout.n_vars, c.pb.num_constraints(), c.pb.n_inputs)
    assert (r.V, r.nC) == {1: (8679, 9145), 4: (8743, 9209)}[msg_len] and r.domain_size == 1 << 14 and pad == 0
    lay = c.layout
    assert lay.mont_adder_var0 - lay.hash_window_var0 == 2 * W and lay.edwards_adder_var0 - lay.converter_var0 == 2 * -(-W // 62)


def test_non_canonical_decomposition_is_rejected():
    """the bits of x + r: field2bits_strict as the reference has it accepts them, BitsNotAbove does not -- alone and in the circuit"""
    e = KATS["eddsa"]
    A, R, s = tuple(int(v) for v in e["A"]), tuple(int(v) for v in e["pure"]["R"]), int(e["pure"]["s"])
    assert A[0] + FR < 1 << 254
    pb = Protoboard()
    x = pb.allocate(A[0])
    g = JG.Field2BitsStrict(pb, x)
    g.generate_r1cs_constraints()
    g.generate_r1cs_witness(A[0] + FR)
    assert pb.is_satisfied()                                           # the gap in the reference's gadget
    rng = JG.BitsNotAbove(pb, g.result(), FR - 1)
    rng.generate_r1cs_constraints()
    rng.generate_r1cs_witness()
    assert not pb.is_satisfied()
    g.generate_r1cs_witness()
    rng.generate_r1cs_witness()
    assert pb.is_satisfied()
    c = pure(4)
    c.assign(A, R, s, b"abcd", bits_value={"ax": A[0] + FR})
    assert [c.pb.val(b) for b in c.core.ax_bits.result()] == field_bits(A[0] + FR, 254) and not c.pb.is_satisfied()
    first_range = 254 + 32 + 25 + 127 * 2 + 126 * 7 + 762 + 253 + 762      # the constraints before BitsNotAbove(bits of A.x)
    dot = lambda lc: sum(k * c.pb.values[i] for i, k in lc.items()) % FR
    bad = [i for i in range(c.pb.num_constraints()) if dot(c.pb.A[i]) * dot(c.pb.B[i]) % FR != dot(c.pb.C[i])]
    assert first_range <= bad[0] < first_range + 253                   # the range check is the first constraint to fail
    c.assign(A, R, s, b"abcd")
    assert c.pb.is_satisfied()


@pytest.mark.parametrize("msg_len", [2, 3])
def test_padding_bits_agree_with_the_verifier(msg_len):
    """508 + 16 and 508 + 24 bits are no multiples of 3: one and two zero padding bits, and the circuit's verdict is jubjub_cases.verify's"""
    c = pure(msg_len)
    assert c.n_pad == {2: 1, 3: 2}[msg_len] and c.layout.pad_bit0 == c.pad_bits[0]
    rng = random.Random(msg_len)
    msg = JC.make_msg("pure", msg_len, rng)
    A, (R, s), _ = JC.sign("pure", msg, rng.randrange(1, JC.L))
    for m, want in ((msg, True), (JC.flip_last("pure", msg), False)):
        w = c.assign(A, R, s, m)
        assert JC.verify("pure", A, (R, s), m) == want == c.pb.is_satisfied() == c.equation_holds() == c.r1cs().is_satisfied(w)
        t = JC.hash_public("pure", R, A, m)
        assert [c.pb.val(b) for b in c.core.hash.result()] == JC.field_bits(t)
    c.assign(A, R, s, msg)
    c.pb.set_val(c.pad_bits[-1], 1)
    assert not c.pb.is_satisfied()
    c.pb.set_val(c.pad_bits[-1], 0)


def test_binding_names_without_a_device():
    """the new capability has names of its own: the layout structure mirrors the namedtuple field for field"""
    from ethsnarks_amd import jubjub as J, prover
    assert [n for n, _ in J.EddsaPureLayout._fields_] == list(JG.PURE_LAYOUT_FIELDS) and len(JG.PURE_LAYOUT_FIELDS) == 26
    assert prover.ABI_VERSION == 9 and "zk_eddsa_fill_pure_witnesses" in prover.EXPORTS
    assert JG.eddsa_pure_circuit(1)[1] == pure(1).layout
