"""What the signer's tests assert on both builds, shared by test_eddsa_sign_emul.py and test_eddsa_sign_gpu.py: every check takes the bindings
(ethsnarks_amd.prover and ethsnarks_amd.jubjub with the emulation or the device library loaded) and compares with eddsa_sign_cases.py.  Exact
comparisons: everything is integer arithmetic."""
import ctypes as C
import random

import numpy as np

from ethsnarks_amd import fields as F
import eddsa_sign_cases as SC
import jubjub_cases as JC
from jubjub_checks import spread

TOP = (1 << 256) - 1


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def wide_limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(64, "little") for v in vals), dtype="<u8").reshape(-1, 8).copy()


def probe(J, op, a, b, c, n, length, out):
    return J._sign_lib().zk_eddsa_sign_probe(op, vp(a), vp(b), vp(c), n, length, 0, vp(out))


# ---------------------------------------------------------------- 1. the probes
def check_probe_sha512(J):
    for length, rows in SC.sha_rows():
        a = np.frombuffer(b"".join(rows), dtype=np.uint8).copy() if length else np.zeros(1, dtype=np.uint8)
        out = np.zeros((len(rows), 64), dtype=np.uint8)
        assert probe(J, 0, a, None, None, len(rows), length, out) == 0, length
        for i, row in enumerate(rows):
            assert bytes(out[i]) == SC.sha_want(row), (length, i)
    rows = [bytes([i]) * 129 for i in range(70)]                       # more than a workgroup
    out = np.zeros((70, 64), dtype=np.uint8)
    assert probe(J, 0, np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), None, None, 70, 129, out) == 0
    assert [bytes(o) for o in out] == [SC.sha_want(r) for r in rows]


def check_probe_mod_l(J):
    vals = SC.mod_l_cases()
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    assert probe(J, 1, wide_limbs(vals), None, None, len(vals), 0, out) == 0
    got = F.limbs_to_ints(out)
    bad = [i for i, v in enumerate(vals) if got[i] != v % SC.L]
    assert not bad, "mod L: %d wrong, the first: case %d, 0x%x" % (len(bad), bad[0], vals[bad[0]])


def check_probe_mod_e(J):
    cases = SC.mod_e_cases()
    arrs = [F.ints_to_limbs([t[i] for t in cases]) for i in range(3)]
    out = np.zeros((len(cases), 4), dtype=np.uint64)
    assert probe(J, 2, arrs[0], arrs[1], arrs[2], len(cases), 0, out) == 0
    got = F.limbs_to_ints(out)
    bad = [i for i, (a, b, c) in enumerate(cases) if got[i] != (a + b * c) % SC.E]
    assert not bad, "mod E: %d wrong, the first: case %d" % (len(bad), bad[0])


# ---------------------------------------------------------------- 2. parity with jubjub_cases.sign
def check_parity(J, scheme, length, items, B=None, n=None):
    use = spread(items, n) if n else items
    with J.EdDSASigner(scheme, B=B, msg_len=length) as sg:
        A, sigs = sg.sign([k for k, _ in use], [m for _, m in use])
    want = [SC.expected(scheme, k, m, B or JC.GENERATOR) for k, m in use]
    bad = [i for i in range(len(use)) if (A[i], sigs[i]) != want[i]]
    assert not bad, "%s, msg_len %d, n = %d: %d wrong, the first: item %d, key 0x%x" % (scheme, length, len(use), len(bad), bad[0], use[bad[0]][0])


def check_lengths(J, scheme):
    for length in SC.LENGTHS[scheme]:
        check_parity(J, scheme, length, SC.length_items(scheme, length))


def check_keys_and_sizes(J, scheme, sizes):
    """the directed keys on their own, then cycled to every batch size with the directed items in the first and the last lanes"""
    items = SC.key_items(scheme)
    check_parity(J, scheme, 3, items)
    for n in sizes:
        check_parity(J, scheme, 3, items, n=n)


def check_other_base(J, scheme):
    check_parity(J, scheme, 3, SC.key_items(scheme)[2:6], B=SC.B2)


# ---------------------------------------------------------------- 3. round trip
def check_round_trip(J, scheme, n):
    items = spread(SC.key_items(scheme), n)
    keys, msgs = [k for k, _ in items], [m for _, m in items]
    flipped = n // 2
    wrong = list(msgs)
    wrong[flipped] = JC.flip_last(scheme, msgs[flipped])
    with J.EdDSASigner(scheme, msg_len=3) as sg:
        A, sigs = sg.sign(keys, msgs)
    with J.EdDSAVerifier(scheme, msg_len=3) as v:
        assert v.verify(A, sigs, msgs) == [True] * n
        assert v.verify(A, sigs, wrong) == [i != flipped for i in range(n)]


def check_round_trip_fill(J, scheme):
    """the device-signed batch through the witness fill of the scheme's circuit"""
    items = SC.key_items(scheme)[1:5]
    n = len(items)
    keys, msgs = [k for k, _ in items], [m for _, m in items]
    wrong = list(msgs)
    wrong[n - 1] = JC.flip_last(scheme, msgs[n - 1])
    with J.EdDSASigner(scheme, msg_len=3) as sg:
        A, sigs = sg.sign(keys, msgs)
    with J.EdDSAVerifier(scheme, msg_len=3) as v:
        fill = v.fill_witnesses if scheme == "mimc" else v.fill_pedersen_witnesses
        verdicts, buf = fill(A, sigs, msgs)
        assert verdicts == [True] * n
        verdicts, _ = fill(A, sigs, wrong, buf)
        assert verdicts == [True] * (n - 1) + [False]
        buf.free()


# ---------------------------------------------------------------- 4. determinism
def raw_sign(J, sg, keys, msgs, fill=0):
    """the C ABI itself: (rc, A, R, s) with the outputs pre-filled"""
    n = len(keys)
    k = F.ints_to_limbs(keys)
    if sg.scheme == "mimc":
        m = F.ints_to_limbs([int(x) for msg in msgs for x in msg])
    else:
        m = np.frombuffer(b"".join(bytes(x) for x in msgs), dtype=np.uint8).copy()
    A = np.full((n, 8), fill, dtype=np.uint64)
    R = np.full((n, 8), fill, dtype=np.uint64)
    s = np.full((n, 4), fill, dtype=np.uint64)
    rc = J._sign_lib().zk_eddsa_sign_batch(sg._h, vp(k), vp(m), n, vp(A), vp(R), vp(s))
    return rc, A, R, s


def check_determinism(J, scheme):
    items = SC.key_items(scheme)
    keys, msgs = [k for k, _ in items], [m for _, m in items]
    perm = list(range(len(items)))
    random.Random(7).shuffle(perm)
    assert perm != sorted(perm)
    with J.EdDSASigner(scheme, msg_len=3) as sg:
        first = raw_sign(J, sg, keys, msgs)
        again = raw_sign(J, sg, keys, msgs, fill=9)
        moved = raw_sign(J, sg, [keys[p] for p in perm], [msgs[p] for p in perm])
    assert first[0] == again[0] == moved[0] == 0
    for a, b, c in zip(first[1:], again[1:], moved[1:]):
        assert a.tobytes() == b.tobytes() and np.array_equal(a[perm], c)


# ---------------------------------------------------------------- 5. errors: ZK_ERR_ARG (1) and nothing written
def check_errors(zk, J):
    lib = J._sign_lib()
    good = SC.key_items("mimc")
    with J.EdDSASigner("mimc", msg_len=3) as sg:
        for n in (2, 3):                                               # the bad key is the last of two or three items
            for bad in SC.BAD_KEYS:
                keys = [k for k, _ in good[:n - 1]] + [bad]
                rc, A, R, s = raw_sign(J, sg, keys, [m for _, m in good[:n]], fill=7)
                assert rc == 1 and (A == 7).all() and (R == 7).all() and (s == 7).all(), (n, bad)
            msgs = [list(m) for _, m in good[:n]]
            msgs[n - 1][2] = JC.Q                                      # a message element = r
            rc, A, R, s = raw_sign(J, sg, [k for k, _ in good[:n]], msgs, fill=7)
            assert rc == 1 and (A == 7).all() and (R == 7).all() and (s == 7).all(), n
        k, m = F.ints_to_limbs([good[0][0]]), F.ints_to_limbs(list(good[0][1]))
        outs = [np.full(8, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64), np.full(4, 7, dtype=np.uint64)]
        for hole in range(6):                                          # each pointer NULL in turn
            args = [sg._h, vp(k), vp(m), vp(outs[0]), vp(outs[1]), vp(outs[2])]
            args[hole] = None
            assert lib.zk_eddsa_sign_batch(args[0], args[1], args[2], 1, args[3], args[4], args[5]) == 1, hole
            assert all((o == 7).all() for o in outs), hole
        assert lib.zk_eddsa_sign_batch(sg._h, vp(k), vp(m), 0, vp(outs[0]), vp(outs[1]), vp(outs[2])) == 0 and all((o == 7).all() for o in outs)
        for bad in SC.BAD_KEYS:
            try:
                sg.sign([good[0][0], bad], [good[0][1], good[1][1]])
                raise AssertionError("key 0x%x was signed with" % bad)
            except zk.ZkError as e:
                assert e.code == 1
        try:
            sg.sign([good[0][0]], [[1, 2, JC.Q]])
            raise AssertionError("a message element = r was signed")
        except zk.ZkError as e:
            assert e.code == 1
        assert sg.sign([], []) == ([], [])
        A, sigs = sg.sign([good[0][0]], [good[0][1]])                  # and the handle still signs
        assert (A[0], sigs[0]) == SC.expected("mimc", *good[0])
    with J.EdDSASigner("pure", msg_len=3) as sg:                       # the key check holds for the byte schemes too
        rc, A, R, s = raw_sign(J, sg, [5, JC.L], [b"abc", b"def"], fill=7)
        assert rc == 1 and (A == 7).all() and (R == 7).all() and (s == 7).all()
    out = np.full(16, 7, dtype=np.uint64)
    a = np.zeros(16, dtype=np.uint64)
    for op in (3, -1, 99):
        assert probe(J, op, a, a, a, 1, 8, out) == 1 and (out == 7).all(), op
    assert probe(J, 0, None, None, None, 1, 8, out) == 1 and probe(J, 1, a, None, None, 1, 0, None) == 1 and (out == 7).all()
    assert probe(J, 2, a, None, a, 1, 0, out) == 1 and probe(J, 2, a, a, None, 1, 0, out) == 1 and (out == 7).all()
    assert probe(J, 1, a, None, None, 0, 0, out) == 0 and (out == 7).all()


# ---------------------------------------------------------------- 6. static
def check_static(zk, J):
    assert zk.ABI_VERSION == 9
    assert "zk_eddsa_sign_batch" in zk.EXPORTS and "zk_eddsa_sign_probe" in zk.EXPORTS
    assert len(J._SYMBOLS) == 13 and not any("sign" in s for s in J._SYMBOLS)
