"""The witness fill of the MiMC-EdDSA circuit on an MI355X (libzkhip.so): the checks of test_eddsa_circuit_emul.py on the device at n = 1, 3 and
65, and three signatures -- two valid, one wrong -- taken from the circuit's keygen through fill_witnesses and submit_batch(device_ptr=...) to
the batch verifier, which accepts exactly the two: the prover refuses the batch that holds the wrong one's row (ZK_ERR_DEGREE), proves the two
items whose verdict is 1 from rows filled side by side in one submit of k = 2, and no proof verifies under the wrong signature's public inputs.  No timing is asserted (tools/eddsa_circuit_bench.py measures)."""
import pytest

import eddsa_circuit_cases as EC
import eddsa_circuit_checks as chk
import jubjub_cases as JC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J(hip):
    from ethsnarks_amd import jubjub
    jubjub._lib()
    return jubjub


@pytest.mark.parametrize("n", EC.SIZES)
def test_rows_and_verdicts(hip, J, n):
    chk.check_rows(hip, J, n)


def test_three_message_elements_and_another_base_point(hip, J):
    chk.check_rows(hip, J, 3, msg_len=3, B=JC.mul(JC.GENERATOR, 77))


def test_refusals(hip, J):
    chk.check_refusals(hip, J)


def test_one_shot_iterables(hip, J):
    chk.check_one_shot_iterables(J)


def test_three_signatures_to_proofs(hip, J):
    d = {c[0]: c for c in EC.directed(1)}
    items = [d["valid"], d["last bit of the message"], d["s + L"]]    # the wrong one has public inputs of its own (another message)
    vk, texts = chk.check_proofs(hip, J, items, [True, False, True])
    ver = hip.Verifier(vk)
    assert ver.verify(texts) == [True, False, True]
    assert [hip.stub_verify(vk.to_json(), t) for t in texts] == [True, False, True]
    ver.close()
