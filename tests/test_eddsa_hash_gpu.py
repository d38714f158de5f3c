"""The witness fill of the EdDSA circuit of the "hash" scheme on an MI355X (libzkhip.so): the checks of test_eddsa_hash_emul.py on the device, and
three signatures of EdDSASigner("hash") -- valid, a wrong message bit, s + L -- taken from the circuit's keygen through fill_hash_witnesses and
submit_batch(device_ptr=...) to the batch verifier, which accepts exactly the valid ones.  No timing is asserted
(tools/eddsa_circuit_bench.py --scheme hash measures)."""
import pytest

import eddsa_hash_cases as HC
import eddsa_hash_checks as chk
import jubjub_cases as JC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J(hip):
    from ethsnarks_amd import jubjub
    jubjub._lib()
    return jubjub


@pytest.mark.parametrize("n", HC.SIZES)
def test_rows_and_verdicts(hip, J, n):
    chk.check_rows(hip, J, n)


def test_no_padding_bit_reference_signature(hip, J):
    chk.check_items(hip, J, [HC.reference_signature()], 3)


def test_two_padding_bits_and_another_base_point(hip, J):
    B = JC.mul(JC.GENERATOR, 77)
    chk.check_items(hip, J, [HC.one_valid(2, B)], 2, B)


def test_second_segment_and_edwards_adder(hip, J):
    chk.check_items(hip, J, [HC.one_valid(HC.TWO_SEGMENT_MSG_LEN)], HC.TWO_SEGMENT_MSG_LEN)


def test_lone_last_window(hip, J):
    chk.check_items(hip, J, [HC.one_valid(HC.LONE_MSG_LEN)], HC.LONE_MSG_LEN)


def test_refusals(hip, J):
    chk.check_refusals(hip, J)


def test_one_shot_iterables(hip, J):
    chk.check_one_shot_iterables(J)


def test_three_signatures_to_proofs(hip, J):
    items = chk.signed_items(J)                                        # the wrong one has public inputs of its own (another message)
    vk, texts = chk.check_proofs(hip, J, items, [True, False, True])
    ver = hip.Verifier(vk)
    assert ver.verify(texts) == [True, False, True]
    assert [hip.stub_verify(vk.to_json(), t) for t in texts] == [True, False, True]
    ver.close()
