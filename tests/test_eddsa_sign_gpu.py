"""The EdDSA signer on an MI355X (libzkhip.so): the checks of test_eddsa_sign_emul.py on the device -- the SHA-512, the Barrett reductions and the
doubling-free fixed-base loop of csrc/eddsa_sign.hpp as gfx950 executes them -- at n = 1, 63, 64, 65 and 130 with the directed keys in the first
and the last lanes; two device-signed messages proven and the proofs accepted; one timed sign call per scheme at n = 2^16 beside the verify call
of the same signatures.  Times are printed, never asserted."""
import ctypes as C
import time
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import eddsa_circuit_checks as ECC
import eddsa_sign_cases as SC
import eddsa_sign_checks as chk
import jubjub_cases as JC

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]
BIG = 1 << 16


@pytest.fixture(scope="module")
def J(hip):
    from ethsnarks_amd import jubjub
    jubjub._sign_lib()
    return jubjub


def test_probe_sha512(J):
    chk.check_probe_sha512(J)


def test_probe_mod_l(J):
    chk.check_probe_mod_l(J)


def test_probe_muladd_mod_e(J):
    chk.check_probe_mod_e(J)


@pytest.mark.parametrize("scheme", SC.SCHEMES)
def test_parity_at_every_message_length(J, scheme):
    chk.check_lengths(J, scheme)


@pytest.mark.parametrize("scheme", SC.SCHEMES)
def test_parity_for_directed_keys_and_batch_sizes(J, scheme):
    chk.check_keys_and_sizes(J, scheme, SIZES)


@pytest.mark.parametrize("scheme", SC.SCHEMES)
def test_parity_on_a_second_base_point(J, scheme):
    chk.check_other_base(J, scheme)


@pytest.mark.parametrize("scheme", SC.SCHEMES)
def test_round_trip_through_the_verifier(J, scheme):
    chk.check_round_trip(J, scheme, 130)


@pytest.mark.parametrize("scheme", ("mimc", "pure"))
def test_round_trip_through_the_witness_fill(J, scheme):
    chk.check_round_trip_fill(J, scheme)


@pytest.mark.parametrize("scheme", SC.SCHEMES)
def test_determinism(J, scheme):
    chk.check_determinism(J, scheme)


def test_errors(hip, J):
    chk.check_errors(hip, J)


def test_static(hip, J):
    chk.check_static(hip, J)


def test_one_launch_whatever_n(hip, J):
    items = SC.key_items("mimc")
    with J.EdDSASigner("mimc", msg_len=3) as sg:
        sg.sign([items[0][0]], [items[0][1]])                          # (the table is built by the first call)
        counts = {}
        for n in (1, 130):
            use = chk.spread(items, n)
            before = hip.launch_count()
            sg.sign([k for k, _ in use], [m for _, m in use])
            counts[n] = hip.launch_count() - before
    assert counts == {1: 1, 130: 1}, counts


def test_two_device_signed_messages_to_proofs(hip, J):
    """sign -> fill witnesses -> prove -> verify, every step on the device; one key generation"""
    pairs = SC.key_items("mimc")[5:7]
    msgs = [m[:1] for _, m in pairs]
    with J.EdDSASigner("mimc", msg_len=1) as sg:
        A, sigs = sg.sign([k for k, _ in pairs], msgs)
    items = [("device-signed", A[i], sigs[i], msgs[i], True) for i in range(2)]
    vk, texts = ECC.check_proofs(hip, J, items, [True, True])
    ver = hip.Verifier(vk)
    assert ver.verify(texts) == [True, True]
    ver.close()


def timed(label, items, fn):
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    print("%-28s n = %d: %8.2f ms, %10.0f items/s" % (label, items, 1e3 * dt, items / dt))


def test_timing_at_2p16(hip, J):
    """one timed sign call per scheme at n = 2^16 and msg_len 3 over 2^16 distinct seeded keys and messages (host checks and copies included;
    the table is built, and each of the three kernels has run, in a one-item call before), the verify call of the same signatures and the SHA-512
    of the same byte count on its own beside it; printed, never asserted"""
    L = J._sign_lib()
    p = chk.vp
    hip._check(L.zk_eddsa_sign_probe(0, p(np.zeros(8, dtype=np.uint8)), None, None, 1, 8, 0, p(np.zeros(64, dtype=np.uint8))))   # (the probe kernel has run once)
    for scheme in SC.SCHEMES:
        rng = np.random.default_rng(17)
        keys = rng.integers(1, 1 << 62, size=(BIG, 4), dtype=np.uint64)
        keys[:, 3] &= np.uint64((1 << 56) - 1)                          # below 2^248 < L, and not 0
        if scheme == "mimc":
            m = rng.integers(0, 1 << 60, size=(BIG, 3 * 4), dtype=np.uint64)   # every element below 2^252 < r
            msg0 = F.limbs_to_ints(m[0].reshape(3, 4))
            sha_len = 32 + 96
        else:
            m = rng.integers(0, 256, size=(BIG, 3), dtype=np.uint8)
            msg0 = bytes(m[0])
            sha_len = 32 + 3 if scheme == "pure" else 96
        assert len(np.unique(keys, axis=0)) == BIG
        A = np.zeros((BIG, 8), dtype=np.uint64)
        R = np.zeros((BIG, 8), dtype=np.uint64)
        s = np.zeros((BIG, 4), dtype=np.uint64)
        verdicts = np.zeros(BIG, dtype=np.uint8)
        with J.EdDSASigner(scheme, msg_len=3) as sg, J.EdDSAVerifier(scheme, msg_len=3) as v:
            hip._check(L.zk_eddsa_sign_batch(sg._h, p(keys[:1].copy()), p(m[:1].copy()), 1, p(A), p(R), p(s)))
            hip._check(L.zk_eddsa_verify_batch(v._h, p(A), p(R), p(s), p(m[:1].copy()), 1, p(verdicts)))   # (both kernels have run once)
            timed("EdDSA sign, %s" % scheme, BIG, lambda: hip._check(L.zk_eddsa_sign_batch(sg._h, p(keys), p(m), BIG, p(A), p(R), p(s))))
            timed("EdDSA verify, %s" % scheme, BIG, lambda: hip._check(L.zk_eddsa_verify_batch(v._h, p(A), p(R), p(s), p(m), BIG, p(verdicts))))
        assert verdicts.all()
        key0 = F.limbs_to_ints(keys[0])[0]
        want = SC.expected(scheme, key0, msg0)
        got = (tuple(F.limbs_to_ints(A[0])), (tuple(F.limbs_to_ints(R[0])), F.limbs_to_ints(s[0])[0]))
        assert got == want
        data = rng.integers(0, 256, size=(BIG, sha_len), dtype=np.uint8)
        out = np.zeros((BIG, 64), dtype=np.uint8)
        timed("SHA-512 of %d bytes alone" % sha_len, BIG, lambda: hip._check(L.zk_eddsa_sign_probe(0, p(data), None, None, BIG, sha_len, 0, p(out))))
