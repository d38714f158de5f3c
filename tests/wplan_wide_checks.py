"""Checks of the wide (lane-parallel) witness plan that run unchanged on the CPU stand-in (test_wplan_wide_emul.py) and on the device
(test_wplan_wide_gpu.py).  `zk` is the ethsnarks_amd.prover module with a library loaded.  The yardsticks are the tape plan from the same
start buffer (byte for byte) and the front end's witness; everything is integer arithmetic and compares exactly."""
import functools
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F, r1cs as R


@functools.lru_cache(maxsize=None)
def case(name):
    """(R1CS, supplied variables, a few front-end witnesses in Montgomery form) -- computed once, never written to"""
    if name == "poseidon_preimage":
        made = [G.poseidon_preimage_circuit(2, seed=7 + p) for p in range(3)]
        supplied = [0, 1, 2, 3]                                        # ONE, digest, the two inputs
    elif name == "poseidon_membership":
        D = 2
        made = [G.poseidon_membership_circuit(D, leaf=1000 + p, address=p, path=[77 + p, 5 * p + 1]) for p in range(3)]
        supplied = list(range(0, 1 + 1 + D + D + 1))                   # ONE, root, address bits, path, leaf
    elif name == "mimc_preimage":
        made = [G.mimc_preimage_circuit(2, seed=70 + p) for p in range(3)]
        supplied = list(range(0, 1 + 1 + 1 + 2))                       # ONE, digest, iv, m[0..1]
    elif name == "chain":
        made = [R.synthetic_chain(2, seed=90 + p) for p in range(3)]
        supplied = [0, 1, 2]
    else:
        raise KeyError(name)
    ws = [F.fr_to_mont(m[1]) for m in made]
    for w in ws:
        w.setflags(write=False)
    return made[0][0], supplied, ws


CASES = ["poseidon_preimage", "poseidon_membership", "mimc_preimage", "chain"]


def start_rows(r, supplied, ws, k):
    """k rows holding the supplied variables only, and one sentinel row after them"""
    start = np.zeros((k + 1, r.V + 1, 4), dtype=np.uint64)
    for p in range(k):
        start[p, supplied] = ws[p % len(ws)][supplied]
    start[k] = np.arange(4 * (r.V + 1), dtype=np.uint64).reshape(r.V + 1, 4) + np.uint64(7)
    return start


def solve_both(zk, tape, wide, start, k):
    out = []
    for plan in (tape, wide):
        buf = zk.DeviceBuffer(start.nbytes)
        buf.upload(start)
        bad = plan.solve(buf.ptr, k)
        out.append((bad, buf.download(start.shape)))
        buf.free()
    return out


def check_parity(zk, name, lanes, ks):
    r, supplied, ws = case(name)
    tape, wide = zk.WitnessPlan(r, supplied), zk.WitnessPlan(r, supplied, lanes=lanes)
    assert wide.info()["kind"] == 1 and wide.info()["lanes"] == lanes and tape.info()["kind"] == 0
    for k in ks:
        start = start_rows(r, supplied, ws, k)
        (bad_t, got_t), (bad_w, got_w) = solve_both(zk, tape, wide, start, k)
        assert bad_t == 0 and bad_w == 0, (k, bad_t, bad_w)
        assert np.array_equal(got_w, got_t), k                          # byte-identical to the tape, sentinel row included
        for p in range(k):
            assert np.array_equal(got_w[p], ws[p % len(ws)]), (k, p)    # the front end's witness
        assert np.array_equal(got_w[k], start[k])
    tape.close(); wide.close()


def check_violations(zk, name, lanes, ks):
    """one supplied variable (variable 1: the digest / root) of one row is wrong: the checks count what the tape's count"""
    r, supplied, ws = case(name)
    tape, wide = zk.WitnessPlan(r, supplied), zk.WitnessPlan(r, supplied, lanes=lanes)
    for k in ks:
        start = start_rows(r, supplied, ws, k)
        victim = k // 2
        start[victim, 1] = F.fr_to_mont([12345])[0]
        (bad_t, got_t), (bad_w, got_w) = solve_both(zk, tape, wide, start, k)
        assert bad_w == bad_t, (k, bad_t, bad_w)
        if name != "chain":                                             # (the chain has no check constraint: variable 1 is an input like any other)
            assert bad_w >= 1
        assert np.array_equal(got_w, got_t), k
        for p in range(k):
            if p != victim:
                assert np.array_equal(got_w[p], ws[p % len(ws)]), (k, p)
    tape.close(); wide.close()


def message(zk, fn):
    with pytest.raises(zk.ZkError) as e:
        fn()
    return e.value.code, str(e.value)


def check_bit_hints(zk, lanes=16):
    k = 3
    cases = [G.field2bits_circuit(253, seed=40 + p) for p in range(k)]
    r, (xv, first, nb) = cases[0][0], cases[0][2]
    supplied = [0, xv, first + nb + 1]                                   # allocation order: x, bits, y, iv, ...
    ws = [F.fr_to_mont(c[1]) for c in cases]
    refused_t = message(zk, lambda: zk.WitnessPlan(r, supplied))
    refused_w = message(zk, lambda: zk.WitnessPlan(r, supplied, lanes=lanes))
    assert refused_w == refused_t and refused_w[0] == 1 and "solved order" in refused_w[1]
    tape = zk.WitnessPlan(r, supplied, bit_hints=[(xv, first, nb)])
    wide = zk.WitnessPlan(r, supplied, bit_hints=[(xv, first, nb)], lanes=lanes)
    start = start_rows(r, supplied, ws, k)
    (bad_t, got_t), (bad_w, got_w) = solve_both(zk, tape, wide, start, k)
    assert bad_t == 0 and bad_w == 0
    assert np.array_equal(got_w, got_t)
    for p in range(k):
        assert np.array_equal(got_w[p], ws[p])
    tape.close(); wide.close()


def check_inv_nonzero_hints(zk, lanes=16):
    vals = [(0, 5, 0, 7, 1), (3, 0, 0, 0, 9), (0, 0, 0, 0, 0)]
    cases = [G.isnonzero_circuit(v) for v in vals]
    r, triples = cases[0][0], cases[0][2]
    iv = max(max(t) for t in triples) + 2                                # allocation order: count, (x, y, m)*, t, iv, ...
    supplied = [0] + [x for x, _, _ in triples] + [iv]
    ws = [F.fr_to_mont(c[1]) for c in cases]
    k = len(cases)
    refused_t = message(zk, lambda: zk.WitnessPlan(r, supplied))
    refused_w = message(zk, lambda: zk.WitnessPlan(r, supplied, lanes=lanes))
    assert refused_w == refused_t and refused_w[0] == 1 and "solved order" in refused_w[1]
    good = dict(inv_hints=[(x, m) for x, _, m in triples], nonzero_hints=[(x, y) for x, y, _ in triples])
    tape, wide = zk.WitnessPlan(r, supplied, **good), zk.WitnessPlan(r, supplied, lanes=lanes, **good)
    start = start_rows(r, supplied, ws, k)
    (bad_t, got_t), (bad_w, got_w) = solve_both(zk, tape, wide, start, k)
    assert bad_t == 0 and bad_w == 0
    assert np.array_equal(got_w, got_t)
    for p in range(k):
        assert np.array_equal(got_w[p], ws[p])
    tape.close(); wide.close()
    # the hints exchanged (Y from the inverse, M from the flag): the checks catch it wherever X is neither 0 nor 1
    swapped = dict(inv_hints=[(x, y) for x, y, _ in triples], nonzero_hints=[(x, m) for x, _, m in triples])
    tape, wide = zk.WitnessPlan(r, supplied, **swapped), zk.WitnessPlan(r, supplied, lanes=lanes, **swapped)
    (bad_t, got_t), (bad_w, got_w) = solve_both(zk, tape, wide, start, k)
    assert bad_w == bad_t and bad_w > 0
    assert np.array_equal(got_w, got_t)
    tape.close(); wide.close()
