"""The witness fill of the MiMC-EdDSA circuit on the CPU emulation build of the HIP sources (csrc/jubjub.hpp k_eddsa_fill, jubjub.cpp): rows
against the front end's generate_r1cs_witness element by element at n = 1, 3 and 65, verdicts against the batch verifier and the integer
restatement, sentinels, refusals, and one chain from the circuit's keygen to a verified proof.  test_eddsa_circuit_gpu.py runs the same checks on
the device.  One lane writes one row and no lanes cooperate, so the emulator's lane order does not enter."""
import ctypes as C

import pytest

import eddsa_circuit_cases as EC
import eddsa_circuit_checks as chk
import jubjub_cases as JC
from test_jubjub_emul import emul_jubjub, zk, J                        # noqa: F401  (the fixtures that build and load the emulation library)


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


@pytest.mark.parametrize("n", EC.SIZES)
def test_rows_and_verdicts(zk, J, n):
    chk.check_rows(zk, J, n)


def test_three_message_elements_and_another_base_point(zk, J):
    chk.check_rows(zk, J, 3, msg_len=3, B=JC.mul(JC.GENERATOR, 77))


def test_refusals(zk, J):
    chk.check_refusals(zk, J)


def test_one_shot_iterables(zk, J):
    chk.check_one_shot_iterables(J)


def test_abi_version(zk):
    assert zk._lib.zk_abi_version() == zk.ABI_VERSION


@pytest.mark.slow
def test_filled_row_proves(zk, J):
    """the whole circuit (no chain shortened), the smallest batch: one valid signature becomes a proof that verifies with A and M as inputs"""
    vk, texts = chk.check_proofs(zk, J, EC.batch(1), [True])
    assert zk.stub_verify(vk.to_json(), texts[0])
