"""The EdDSA signer on the CPU emulation build of the HIP sources (csrc/eddsa_sign.hpp, jubjub.cpp): the SHA-512 and the two wide reductions on
their own against hashlib and Python's %, EdDSASigner.sign against jubjub_cases.sign value for value for every scheme, message length, directed
key, base point and batch size of eddsa_sign_cases.py, the round trip through the verifier and the witness fills, and every refusal with its
outputs proven untouched.  test_eddsa_sign_gpu.py runs the same checks on the device."""
import ctypes as C
import os
import subprocess
import pytest
import eddsa_sign_cases as SC
import eddsa_sign_checks as chk

SIZES = [1, 63, 64, 65, 70]


@pytest.fixture(scope="module")
def emul_jubjub(emul):
    from conftest import ROOT
    d = os.path.join(ROOT, "tests", "emul_jubjub")
    so = os.path.join(d, "libzkhip_emul_jubjub.so")
    csrc = os.path.join(ROOT, "ethsnarks_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith("pp")] + [emul, os.path.join(d, "Makefile")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", d, "-s"])
    return so


@pytest.fixture(scope="module")
def zk(emul_jubjub):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul_jubjub)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    prover._lib = None
    prover._lib_path_loaded = None


@pytest.fixture(scope="module")
def J(zk):
    from ethsnarks_amd import jubjub
    jubjub._sign_lib()
    return jubjub


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


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
    chk.check_round_trip(J, scheme, 9)


@pytest.mark.parametrize("scheme", ("mimc", "pure"))
def test_round_trip_through_the_witness_fill(J, scheme):
    chk.check_round_trip_fill(J, scheme)


@pytest.mark.parametrize("scheme", SC.SCHEMES)
def test_determinism(J, scheme):
    chk.check_determinism(J, scheme)


def test_errors(zk, J):
    chk.check_errors(zk, J)


def test_static(zk, J):
    chk.check_static(zk, J)
