"""The witness fill of the PureEdDSA circuit on an MI355X (libzkhip.so): the checks of test_eddsa_pure_emul.py on the device, and three
signatures -- valid, a wrong message bit, s + L -- taken from the circuit's keygen through fill_pedersen_witnesses and
submit_batch(device_ptr=...) to the batch verifier, which accepts exactly the valid ones.  No timing is asserted
(tools/eddsa_circuit_bench.py --scheme pure measures)."""
import pytest

import eddsa_pure_cases as PC
import eddsa_pure_checks as chk
import jubjub_cases as JC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J(hip):
    from ethsnarks_amd import jubjub
    jubjub._lib()
    return jubjub


@pytest.mark.parametrize("n", PC.SIZES)
def test_rows_and_verdicts(hip, J, n):
    chk.check_rows(hip, J, n)


def test_padding_bit_and_another_base_point(hip, J):
    chk.check_rows(hip, J, 3, msg_len=2, B=JC.mul(JC.GENERATOR, 77))


def test_reference_signature(hip, J):
    chk.check_items(hip, J, [PC.reference_signature()], 4)


def test_lone_last_window(hip, J):
    chk.check_items(hip, J, [PC.long_message()], PC.LONG_MSG_LEN)


def test_refusals(hip, J):
    chk.check_refusals(hip, J)


def test_one_shot_iterables(hip, J):
    chk.check_one_shot_iterables(J)


def test_three_signatures_to_proofs(hip, J):
    d = {c[0]: c for c in PC.directed(1)}
    items = [d["valid"], d["last bit of the message"], d["s + L"]]    # the wrong one has public inputs of its own (another message)
    vk, texts = chk.check_proofs(hip, J, items, [True, False, True])
    ver = hip.Verifier(vk)
    assert ver.verify(texts) == [True, False, True]
    assert [hip.stub_verify(vk.to_json(), t) for t in texts] == [True, False, True]
    ver.close()
