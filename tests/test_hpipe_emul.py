"""The H pipeline on the CPU emulation build of the HIP sources, through its two probes (hpipe_cases.py, hpipe_checks.py): zk_ntt_probe -- one
ntt_run (k_ntt_pass) with the batch, stride, post_alt / alt_from, in2 and sub of a proof, at every size up to 2^14 that selects another
pass plan -- and zk_ctx_probe_h -- every buffer that enqueue_compute_h and enqueue_compute_h4 leave (k_hl_product, k_hl_tail: the
workgroups' shares of the degree check and h[m-1] of every proof of a batch), by value -- and the refusal of a batch whose middle witness
is wrong.  The references themselves are tested here, without any library: the two transform references against each other, the H
reference against the oracle's witness map.  test_hpipe_gpu.py runs the same checks on the device, and the three-pass size 2^21.

Measured on the stand-in, 304 tests in 240 s.  The 273 transform cases take 55 s together, none more than 0.5 s (2^13 with five vectors: the
big-int reference).  The H pipeline takes the rest, nearly all of it in building contexts and proving: the first test on a context pays for
its tables -- four transforms 62 s at 4 096, 34 s at 2 048, 4 s at 256; six transforms 24 s, 12 s, 1.6 s -- and a stage test on a context
that exists takes under 1 s.  The refusal tests prove two batches of three: 7 - 19 s.  So everything on the domains 2 048 and 4 096 and every
refusal test is marked slow; the stages at 256 on both pipelines, the probes' refusals (4 s each) and all transform cases are not."""
import ctypes as C
import pytest
import hpipe_cases as cases
import hpipe_checks as chk


@pytest.fixture(scope="module")
def zk(emul):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    chk.release(prover)
    prover._lib = None
    prover._lib_path_loaded = None


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


def test_transform_references_agree(oracle):
    chk.check_references_agree(oracle)


@pytest.mark.parametrize("name", list(cases.SYSTEMS))
def test_h_reference_is_the_oracles_witness_map(oracle, name):
    chk.check_reference_against_oracle(oracle, name)


@pytest.mark.parametrize("name", cases.EMUL_NTT_CASES)
def test_one_transform_call(zk, oracle, name):
    chk.check_ntt_case(zk, oracle, name)


def test_transform_probe_refusals(zk):
    chk.check_ntt_refusals(zk)


SLOW_SYSTEMS = ("m2048", "m4096")                # the stand-in builds their contexts in 12 - 62 s; whichever test comes first pays


def _marks(name, six, always=False):
    return [pytest.mark.slow] if always or name in SLOW_SYSTEMS else []


@pytest.mark.parametrize("name,batch,six", [pytest.param(n, b, s, marks=_marks(n, s), id="%s-%s-%s" % (n, b, "six" if s else "four"))
                                            for n in cases.SYSTEMS for b in cases.BATCHES for s in (False, True)])
def test_every_stage_of_the_h_pipeline(zk, oracle, monkeypatch, name, batch, six):
    chk.check_h_stages(zk, oracle, monkeypatch, name, batch, six)


@pytest.mark.parametrize("name,six", [pytest.param(n, s, marks=_marks(n, s, always=True), id="%s-%s" % (n, "six" if s else "four")) for n in cases.SYSTEMS for s in (False, True)])
def test_a_wrong_middle_witness_is_refused_and_the_context_proves_on(zk, oracle, monkeypatch, name, six):
    chk.check_degree_refusal(zk, oracle, monkeypatch, name, six)


@pytest.mark.parametrize("six", [False, True], ids=["four", "six"])
def test_h_probe_refusals(zk, oracle, monkeypatch, six):
    chk.check_h_refusals(zk, oracle, monkeypatch, six)
