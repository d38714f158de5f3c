"""Directed batches for the witness fill of the MiMC-EdDSA circuit (zk_eddsa_fill_witnesses): jubjub_cases.signature_cases("mimc", ..) -- valid, wrong
but well-formed, identity and low-order keys, s + L, off-curve A and R -- and s = 2^254.  The expected row of an item is the front end's own
generate_r1cs_witness (jubjub_gadgets.EddsaMimcCircuit.assign), the expected verdict jubjub_cases.verify on Python integers; never the kernel."""
import jubjub_cases as JC
from ethsnarks_amd import jubjub_gadgets as JG

TWO254 = 1 << 254
MALFORMED = ("off-curve A", "off-curve R", "s = 2^254")             # verdict 0, the row keeps what it held
SIZES = [1, 3, 65]                                                  # one lane; a few; one more than a workgroup of 64 (the tail lane alone in its wave)


def directed(msg_len, B=JC.GENERATOR):
    """[(label, A, (R, s), msg, verdict)], the last one a valid item: at n = 65 it is the lone lane of the second workgroup"""
    cases = JC.signature_cases("mimc", msg_len, B)
    valid = cases[0]
    cases = cases[:-1] + [("s = 2^254", valid[1], (valid[2][0], TWO254), valid[3], False), cases[-1]]
    labels = [c[0] for c in cases]
    assert set(MALFORMED) <= set(labels) and labels[0] == "valid" and labels[-1] == "s + L" and cases[-1][4]
    assert {"s + 1", "A = R = identity, s = 0", "low-order A"} <= set(labels)
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


_ROWS = {}


def expected_row(circuit, item):
    """the front end's witness of a well-formed item (computed once per item and circuit)"""
    label, A, (R, s), msg, _ = item
    key = (id(circuit), A, R, s, tuple(msg))
    if key not in _ROWS:
        _ROWS[key] = circuit.assign(A, R, s, msg)
    return _ROWS[key]
