"""The witness fill of the PureEdDSA circuit on the CPU emulation build of the HIP sources (csrc/jubjub.hpp k_eddsa_fill_pure, jubjub.cpp): rows
against the front end's generate_r1cs_witness element by element at n = 1, 3 and 65, a batch with padding bits and another base point, the
reference's own signature, a message whose hash ends in a lone window, verdicts, sentinels, refusals, and one chain from the circuit's keygen to
a verified proof.  test_eddsa_pure_gpu.py runs the same checks on the device.  One lane writes one row and no lanes cooperate, so the emulator's
lane order does not enter."""
import ctypes as C

import pytest

import eddsa_pure_cases as PC
import eddsa_pure_checks as chk
import jubjub_cases as JC
from test_jubjub_emul import emul_jubjub, zk, J                        # noqa: F401  (the fixtures that build and load the emulation library)


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


@pytest.mark.parametrize("n", PC.SIZES)
def test_rows_and_verdicts(zk, J, n):
    chk.check_rows(zk, J, n)


def test_padding_bit_and_another_base_point(zk, J):
    chk.check_rows(zk, J, 3, msg_len=2, B=JC.mul(JC.GENERATOR, 77))


def test_reference_signature(zk, J):
    chk.check_items(zk, J, [PC.reference_signature()], 4)


def test_lone_last_window(zk, J):
    chk.check_items(zk, J, [PC.long_message()], PC.LONG_MSG_LEN)


def test_refusals(zk, J):
    chk.check_refusals(zk, J)


def test_one_shot_iterables(zk, J):
    chk.check_one_shot_iterables(J)


def test_abi_version(zk):
    assert zk._lib.zk_abi_version() == zk.ABI_VERSION == 9


@pytest.mark.slow
def test_filled_row_proves(zk, J):
    """the whole circuit, the smallest batch: one valid signature becomes a proof that verifies with A and the message bits as inputs"""
    vk, texts = chk.check_proofs(zk, J, PC.batch(1), [True])
    assert zk.stub_verify(vk.to_json(), texts[0])
