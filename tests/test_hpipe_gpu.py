"""The H pipeline on the device through its two probes (hpipe_cases.py, hpipe_checks.py): zk_ntt_probe -- one ntt_run with the batch, stride,
post_alt / alt_from, in2 and sub of a proof, at every size that selects another pass plan, the three-pass size 2^21 included -- against
Python integers and, from 2^14, the oracle's transform; zk_ctx_probe_h -- every buffer the six- and the four-transform pipeline leave, the
workgroups' shares of the degree check and h[m-1] of every proof of a batch, by value -- and the refusal of a batch whose middle witness
is wrong.  test_hpipe_emul.py runs the same checks on the CPU stand-in.

Measured on an MI355X: 302 tests in 10.0 s.  The two cases at 2^21 are the slowest, 1.6 s (every fused step, two vectors: 1 GiB of tables and
arrays uploaded, the oracle's reference) and 0.75 s; the first stage test on each four-transform context 0.3 - 0.6 s (its tables), every
other test below 0.3 s, a transform case up to 2^13 below 0.2 s (the big-int reference)."""
import pytest
import hpipe_cases as cases
import hpipe_checks as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_contexts(hip):
    yield
    chk.release(hip)


@pytest.mark.parametrize("name", list(cases.NTT_CASES))
def test_one_transform_call(hip, oracle, name):
    chk.check_ntt_case(hip, oracle, name)


def test_transform_probe_refusals(hip):
    chk.check_ntt_refusals(hip)


@pytest.mark.parametrize("six", [False, True], ids=["four", "six"])
@pytest.mark.parametrize("batch", list(cases.BATCHES))
@pytest.mark.parametrize("name", list(cases.SYSTEMS))
def test_every_stage_of_the_h_pipeline(hip, oracle, monkeypatch, name, batch, six):
    chk.check_h_stages(hip, oracle, monkeypatch, name, batch, six)


@pytest.mark.parametrize("six", [False, True], ids=["four", "six"])
@pytest.mark.parametrize("name", list(cases.SYSTEMS))
def test_a_wrong_middle_witness_is_refused_and_the_context_proves_on(hip, oracle, monkeypatch, name, six):
    chk.check_degree_refusal(hip, oracle, monkeypatch, name, six)


@pytest.mark.parametrize("six", [False, True], ids=["four", "six"])
def test_h_probe_refusals(hip, oracle, monkeypatch, six):
    chk.check_h_refusals(hip, oracle, monkeypatch, six)
