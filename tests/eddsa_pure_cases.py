"""Directed batches for the witness fill of the PureEdDSA circuit (zk_eddsa_fill_pure_witnesses): jubjub_cases.signature_cases("pure", ..) -- valid,
wrong but well-formed, identity and low-order keys, s + L, off-curve A and R -- and s = 2^254; the reference's own signature of b"abcd"
(tests/golden/pedersen_gadget_kats.json); and one message of 53 bytes, whose hash has 311 windows: five full segments and a lone sixth window.
The expected row of an item is the front end's own generate_r1cs_witness (jubjub_gadgets.EddsaPureCircuit.assign), the expected verdict
jubjub_cases.verify on Python integers; never the kernel."""
import json
import os
import random

import jubjub_cases as JC

TWO254 = 1 << 254
MALFORMED = ("off-curve A", "off-curve R", "s = 2^254")             # verdict 0, the row keeps what it held
SIZES = [1, 3, 65]                                                  # one lane; a few; one more than a workgroup of 64 (the tail lane alone in its wave)
LONG_MSG_LEN = 53                                                   # (508 + 424) / 3 = 310.67 -> 311 windows = 5 x 62 + 1
assert (508 + 8 * LONG_MSG_LEN + 2) // 3 == 5 * 62 + 1

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pedersen_gadget_kats.json")) as _f:
    KATS = json.load(_f)


def directed(msg_len, B=JC.GENERATOR):
    """[(label, A, (R, s), msg, verdict)], the last one a valid item: at n = 65 it is the lone lane of the second workgroup"""
    cases = JC.signature_cases("pure", msg_len, B)
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
    """the PureEdDSA signature of b"abcd" in the reference's test_jubjub_eddsa.cpp, as an item"""
    e = KATS["eddsa"]
    A, R = tuple(int(v) for v in e["A"]), tuple(int(v) for v in e["pure"]["R"])
    item = ("reference", A, (R, int(e["pure"]["s"])), e["pure"]["msg"].encode("ascii"), True)
    assert JC.verify("pure", item[1], item[2], item[3])
    return item


def long_message():
    """a valid signature over LONG_MSG_LEN bytes"""
    rng = random.Random(53)
    msg = JC.make_msg("pure", LONG_MSG_LEN, rng)
    A, sig, _ = JC.sign("pure", msg, rng.randrange(1, JC.L))
    assert sig[1] < TWO254 and JC.verify("pure", A, sig, msg)
    return ("long", A, sig, msg, True)


_ROWS = {}


def expected_row(circuit, item):
    """the front end's witness of a well-formed item (computed once per item and circuit)"""
    label, A, (R, s), msg, _ = item
    key = (id(circuit), A, R, s, bytes(msg))
    if key not in _ROWS:
        _ROWS[key] = circuit.assign(A, R, s, msg)
    return _ROWS[key]
