"""The R1CS row evaluation on the device (k_spmv_rows, k_spmv_long_chunks, k_spmv_long_finish behind DevCsr::upload / enqueue) on the systems
with directed row shapes of rowshape_cases.py: every row of every matrix of one and of three witnesses against Python dot products
(zk_ctx_probe_rows), the witness map, proof bytes with four and with six transforms, the refusal, the probe's refusals -- on contexts of
the default path (four transforms) wherever the path is not the parameter.  test_rowshape_emul.py and rowshape_checks.py document the
checks.  Domains of at most 512, at most 3 x 10^5 non-zeros: a test takes seconds, most of them in the big-int reference, which is computed
once per system."""
import pytest
import rowshape_cases as cases
import rowshape_checks as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_contexts(hip):
    yield
    chk.release(hip)


@pytest.mark.parametrize("name", cases.ROW_CASES)
def test_rows_are_the_dot_products(hip, oracle, name):
    chk.check_rows(hip, oracle, name)


@pytest.mark.parametrize("name", cases.ROW_CASES)
def test_rows_of_edge_witnesses_and_canonical_input(hip, oracle, name):
    chk.check_edge_witnesses(hip, oracle, name)


@pytest.mark.parametrize("name", cases.ROW_CASES)
def test_witness_map_is_the_oracles(hip, oracle, name):
    chk.check_witness_map(hip, oracle, name)


@pytest.mark.parametrize("six", [False, True], ids=["four", "six"])
@pytest.mark.parametrize("name", cases.PROOF_CASES)
def test_proof_bytes_are_the_oracles(hip, oracle, name, six):
    chk.check_proofs(hip, oracle, name, six)


@pytest.mark.parametrize("six", [False, True], ids=["four", "six"])
def test_a_witness_wrong_in_a_later_chunk_is_refused(hip, oracle, six):
    chk.check_refusal(hip, oracle, six)


def test_probe_refusals(hip, oracle):
    chk.check_probe_refusals(hip, oracle)
