"""Baby JubJub on an MI355X (libzkhip.so): the checks of test_jubjub_emul.py on the device -- the loose-domain formulas of csrc/jubjub.hpp as
gfx950 executes them -- at n = 1, 63, 64, 65 and 130 (one lane, one short of a wave, a wave, one over, two workgroups and a bit) with the directed
items in the first and the last lanes; 130-signature batches against the restatement item by item; the launch count; one timed run per kernel at
n = 2^16.  Times are printed, never asserted."""
import ctypes as C
import time
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import jubjub_cases as JC
import jubjub_checks as chk

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]
BIG = 1 << 16


@pytest.fixture(scope="module")
def J(hip):
    from ethsnarks_amd import jubjub
    jubjub._lib()
    return jubjub


def test_constants_and_pinned_values(J):
    chk.check_constants(J)
    chk.check_kats(J)
    chk.check_hash_to_point(J)


def test_point_operations(J):
    chk.check_point_ops(J, 20, SIZES)


def test_scalar_multiplication(J):
    chk.check_scalar_mul(J, 20, SIZES)


def test_pedersen(J):
    chk.check_pedersen(J, SIZES)
    chk.check_tables(J)


@pytest.mark.parametrize("scheme", chk.SCHEMES)
def test_signatures(J, scheme):
    chk.check_signatures(J, scheme, SIZES)


def test_cross_scheme(J):
    chk.check_cross_scheme(J)


@pytest.mark.parametrize("scheme", chk.SCHEMES)
def test_batch_parity(J, scheme):
    """valid and invalid items interleaved: no wave is uniform"""
    A, sigs, msgs, want = JC.batch(scheme, 3, 130)
    with J.EdDSAVerifier(scheme, msg_len=3) as v:
        assert v.verify(A, sigs, msgs) == want


def test_off_curve_points_are_refused(hip, J):
    with pytest.raises(hip.ZkError) as e:
        J.scalar_mul([JC.GENERATOR] * 64 + [JC.OFF_CURVE], [3] * 65)
    assert e.value.code == 1
    with pytest.raises(hip.ZkError) as e:
        J.point_add([JC.OFF_CURVE] + [JC.GENERATOR] * 64, [JC.GENERATOR] * 65)
    assert e.value.code == 1


def tile(points, n):
    a = F.ints_to_limbs([c for p in points for c in p]).reshape(-1, 8)
    return np.ascontiguousarray(np.tile(a, (n // len(points), 1)))


def test_launch_count_does_not_grow_with_n(hip, J):
    pts64 = JC.random_points(64, 41)
    ks = F.ints_to_limbs([(i * 0x9E3779B97F4A7C15FFFF + 7) ** 4 % (1 << 256) for i in range(64)])
    counts = {}
    with J.PedersenHasher(b"test", 3 * 62) as h, J.EdDSAVerifier("mimc", msg_len=1) as v:
        sig = chk.sig_cases("mimc", 1)[0]
        for n in (1, 4096):
            p = tile(pts64, max(n, 64))[:n].copy()
            k = np.ascontiguousarray(np.tile(ks, (max(n, 64) // 64, 1))[:n])
            out = np.zeros((n, 8), dtype=np.uint64)
            before = hip.launch_count()
            hip._check(hip._lib.zk_jj_scalar_mul(hip._p64(p), hip._p64(k), C.c_uint32(n), 0, hip._p64(out)))
            hip._check(hip._lib.zk_jj_point_op(0, hip._p64(p), hip._p64(p), C.c_uint32(n), 0, hip._p64(out)))
            h.hash_windows([[i % 8 for i in range(62)]] * n)
            v.verify([sig[1]] * n, [sig[2]] * n, [sig[3]] * n)
            counts[n] = hip.launch_count() - before
    assert counts[1] == counts[4096] == 4, counts


def timed(label, items, fn, unit):
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    print("%-28s n = %d: %8.2f ms, %10.0f %s/s" % (label, items, 1e3 * dt, items / dt, unit))


def test_timing_at_2p16(hip, J):
    """one timed run per kernel at n = 2^16 (host staging and copies included); printed, never asserted"""
    L = hip._lib
    pts64 = JC.random_points(64, 43)
    p = tile(pts64, BIG)
    rng = np.random.default_rng(5)
    k = rng.integers(0, 1 << 63, size=(BIG, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    out = np.zeros((BIG, 8), dtype=np.uint64)
    timed("scalar multiplication", BIG, lambda: hip._check(L.zk_jj_scalar_mul(hip._p64(p), hip._p64(k), C.c_uint32(BIG), 0, hip._p64(out))), "mul")
    assert F.limbs_to_ints(out[:1]) + F.limbs_to_ints(out[1:2]) != [0, 0]
    timed("point addition", BIG, lambda: hip._check(L.zk_jj_point_op(0, hip._p64(p), hip._p64(p), C.c_uint32(BIG), 0, hip._p64(out))), "add")
    with J.PedersenHasher(b"test", 3 * 254) as h:
        win = rng.integers(0, 8, size=(BIG, 254), dtype=np.uint8)
        timed("Pedersen hash, 254 windows", BIG,
              lambda: hip._check(L.zk_pedersen_hash(h._h, win.ctypes.data_as(C.c_void_p), None, 254, BIG, out.ctypes.data_as(C.c_void_p))), "hash")
        first = F.limbs_to_ints(out[0])
        assert (first[0], first[1]) == JC.pedersen_windows(b"test", [int(w) for w in win[0]])
    for scheme in chk.SCHEMES:
        length = 3
        r = np.random.default_rng(6)
        import random
        prng = random.Random(8)
        t0 = time.perf_counter()
        signed = [JC.sign(scheme, JC.make_msg(scheme, length, prng), prng.randrange(1, JC.L)) for _ in range(64)]
        t_sign = (time.perf_counter() - t0) / 64
        t0 = time.perf_counter()
        assert all(JC.verify(scheme, a, sig, m) for a, sig, m in signed[:4])
        t_ver = (time.perf_counter() - t0) / 4
        A = tile([a for a, _, _ in signed], BIG)
        R = tile([sig[0] for _, sig, _ in signed], BIG)
        s = np.ascontiguousarray(np.tile(F.ints_to_limbs([sig[1] for _, sig, _ in signed]), (BIG // 64, 1)))
        if scheme == "mimc":
            m = np.ascontiguousarray(np.tile(F.ints_to_limbs([x for _, _, msg in signed for x in msg]).reshape(64, -1), (BIG // 64, 1)))
        else:
            m = np.ascontiguousarray(np.tile(np.frombuffer(b"".join(msg for _, _, msg in signed), dtype=np.uint8).reshape(64, length), (BIG // 64, 1)))
        verdicts = np.zeros(BIG, dtype=np.uint8)
        with J.EdDSAVerifier(scheme, msg_len=length) as v:
            timed("EdDSA verify, %s" % scheme, BIG,
                  lambda: hip._check(L.zk_eddsa_verify_batch(v._h, *[a.ctypes.data_as(C.c_void_p) for a in (A, R, s, m)], BIG, verdicts.ctypes.data_as(C.c_void_p))), "sig")
        assert verdicts.all()
        print("    the Python restatement: %.1f ms per signature, %.1f ms per verification" % (1e3 * t_sign, 1e3 * t_ver))
