"""Directed batches for the witness fill of the EdDSA circuit of the "hash" scheme (zk_eddsa_fill_hash_witnesses): jubjub_cases.signature_cases("hash", ..)
-- valid, wrong but well-formed, identity and low-order keys, s + L, off-curve A and R -- and s = 2^254, laid out as eddsa_pure_cases.batch lays
its own out; the reference's own signature of b"abc" (tests/golden/pedersen_gadget_kats.json: three bytes, no padding bit); and one valid
signature per shape of the message hash: two segments with one Edwards adder (24 bytes) and three full segments with a lone fourth window (70).
The expected row of an item is the front end's own generate_r1cs_witness (jubjub_gadgets.EddsaHashCircuit.assign), the expected verdict
jubjub_cases.verify on Python integers; never the kernel."""
import random

import eddsa_pure_cases as PC
import jubjub_cases as JC

TWO254 = PC.TWO254
MALFORMED = PC.MALFORMED                                            # verdict 0, the row keeps what it held
SIZES = PC.SIZES                                                    # one lane; a few; the tail lane alone in the second workgroup
KATS = PC.KATS


def msg_windows(msg_len):
    return -(-8 * msg_len // 3)


def msg_pad_bits(msg_len):
    return -8 * msg_len % 3


TWO_SEGMENT_MSG_LEN = 24                                            # 192 bits = 64 windows = 62 + 2: a second segment, ONE Edwards adder, no padding
LONE_MSG_LEN = 70                                                   # 560 bits -> 187 windows = 3 x 62 + 1, one padding bit
assert msg_windows(1) == 3 and msg_pad_bits(1) == 1 and msg_windows(2) == 6 and msg_pad_bits(2) == 2 and msg_windows(3) == 8 and msg_pad_bits(3) == 0
assert msg_windows(23) == 62 and msg_windows(TWO_SEGMENT_MSG_LEN) == 62 + 2 and msg_pad_bits(TWO_SEGMENT_MSG_LEN) == 0
assert msg_windows(LONE_MSG_LEN) == 3 * 62 + 1 and msg_pad_bits(LONE_MSG_LEN) == 1
assert all(msg_windows(n) % 62 != 1 for n in range(1, LONE_MSG_LEN))   # the smallest msg_len whose hash ends in a lone window
assert 254 == 4 * 62 + 6                                            # the RAM hash of this scheme: 254 windows, 62 + 62 + 62 + 62 + 6, never a lone one
# the argument of DESIGN 5m rests on base points of prime order L: those the cases below walk
assert all(JC.basepoint(JC.MSG, i) != JC.IDENTITY and JC.mul(JC.basepoint(JC.MSG, i), JC.L) == JC.IDENTITY for i in range(4))


def directed(msg_len, B=JC.GENERATOR):
    """[(label, A, (R, s), msg, verdict)], the last one a valid item: at n = 65 it is the lone lane of the second workgroup"""
    cases = JC.signature_cases("hash", msg_len, B)
    valid = cases[0]
    cases = cases[:-1] + [("s = 2^254", valid[1], (valid[2][0], TWO254), valid[3], False), cases[-1]]
    labels = [c[0] for c in cases]
    assert set(MALFORMED) <= set(labels) and labels[0] == "valid" and labels[-1] == "s + L" and cases[-1][4]
    assert {"s + 1", "A = R = identity, s = 0", "low-order A", "last bit of the message"} <= set(labels)
    assert all(c[2][1] < TWO254 for c in cases if c[0] != "s = 2^254")
    return cases


def batch(n, msg_len=1, B=JC.GENERATOR):
    """n items: n = 1 a valid one; n = 3 valid, wrong, off-curve; otherwise the directed cases in turn, so that malformed items sit between full rows"""
    d = directed(msg_len, B)
    by = {c[0]: c for c in d}
    if n == 1:
        return [by["valid"]]
    if n == 3:
        return [by["valid"], by["s + 1"], by["off-curve A"]]
    items = [d[i % len(d)] for i in range(n)]
    assert n < 64 or (items[n - 1][0] not in MALFORMED and {c[0] for c in items} == set(by))
    return items


def reference_signature():
    """the EdDSA signature of b"abc" in the reference's test_jubjub_eddsa.cpp, as an item"""
    e = KATS["eddsa"]
    A, R = tuple(int(v) for v in e["A"]), tuple(int(v) for v in e["hash"]["R"])
    item = ("reference", A, (R, int(e["hash"]["s"])), e["hash"]["msg"].encode("ascii"), True)
    assert len(item[3]) == 3 and JC.verify("hash", item[1], item[2], item[3])
    return item


def one_valid(msg_len, B=JC.GENERATOR):
    """a valid signature over msg_len bytes under the base point B"""
    rng = random.Random(1000 + msg_len)
    msg = JC.make_msg("hash", msg_len, rng)
    A, sig, _ = JC.sign("hash", msg, rng.randrange(1, JC.L), B)
    assert sig[1] < TWO254 and JC.verify("hash", A, sig, msg, B)
    return ("valid, %d bytes" % msg_len, A, sig, msg, True)


def non_canonical_forgery():
    """(A, (R, s), msg, M.x): a one-byte message whose M.x + r still has 254 bits, and the signature of the SAME key, nonce and message made
    with t' = H(R, A, the bits of M.x + r) in the place of t.  The reference's constraints, which pin the bits of M.x only up to a multiple of
    r, accept it as a second signature of that message; the verifier does not"""
    rng = random.Random(254)
    key, nonce = rng.randrange(1, JC.L), rng.randrange(1, JC.L)
    msg = next(bytes([b]) for b in range(256) if JC.pedersen_bytes(JC.MSG, bytes([b]))[0] + JC.Q < TWO254)
    mx = JC.pedersen_bytes(JC.MSG, msg)[0]
    A, R = JC.mul(JC.GENERATOR, key), JC.mul(JC.GENERATOR, nonce)
    bits = lambda v: [(v >> i) & 1 for i in range(254)]
    t_forged = JC.pedersen_bits(JC.RAM, bits(R[0]) + bits(A[0]) + bits(mx + JC.Q))[0]
    s = (nonce + key * t_forged) % JC.E
    assert s < TWO254 and t_forged != JC.hash_public("hash", R, A, msg) and not JC.verify("hash", A, (R, s), msg)
    return A, (R, s), msg, mx


_ROWS = {}


def expected_row(circuit, item):
    """the front end's witness of a well-formed item (computed once per item and circuit)"""
    label, A, (R, s), msg, _ = item
    key = (id(circuit), A, R, s, bytes(msg))
    if key not in _ROWS:
        _ROWS[key] = circuit.assign(A, R, s, msg)
    return _ROWS[key]
