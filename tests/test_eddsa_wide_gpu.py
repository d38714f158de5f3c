"""The witness fill of the MiMC-EdDSA circuit with 2 and 4 lanes per signature on an MI355X (libzkhip.so, k_eddsa_fill_wide): the checks of
test_eddsa_wide_emul.py on the device, and three signatures -- valid, wrong message, s + L -- filled with four lanes each and taken through
submit_batch(device_ptr=...) to the batch verifier, with the expectations of test_eddsa_circuit_gpu.py::test_three_signatures_to_proofs.  No
timing is asserted (tools/eddsa_circuit_bench.py --lanes measures)."""
import pytest

import eddsa_circuit_cases as EC
import eddsa_wide_checks as chk
import jubjub_cases as JC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J(hip):
    from ethsnarks_amd import jubjub
    jubjub._lib()
    return jubjub


@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("lanes", chk.WIDE)
def test_rows_and_verdicts(hip, J, lanes, n):
    chk.check_rows(hip, J, n, lanes)


@pytest.mark.parametrize("lanes", chk.WIDE)
def test_a_workgroup_without_a_live_witness(hip, J, lanes):
    chk.check_dead_workgroup(hip, J, lanes)


def test_three_message_elements_and_another_base_point(hip, J):
    chk.check_rows(hip, J, 3, 4, msg_len=3, B=JC.mul(JC.GENERATOR, 77))


def test_same_bytes_as_one_lane(hip, J):
    chk.check_same_bytes_as_one_lane(hip, J)


def test_refusals(hip, J):
    chk.check_refusals(hip, J)


def test_three_signatures_to_proofs(hip, J):
    d = {c[0]: c for c in EC.directed(1)}
    items = [d["valid"], d["last bit of the message"], d["s + L"]]    # the wrong one has public inputs of its own (another message)
    vk, texts = chk.check_proofs(hip, J, items, [True, False, True], lanes=4)
    ver = hip.Verifier(vk)
    assert ver.verify(texts) == [True, False, True]
    assert [hip.stub_verify(vk.to_json(), t) for t in texts] == [True, False, True]
    ver.close()
