"""The R1CS row evaluation (DevCsr::upload / enqueue, k_spmv_rows, k_spmv_long_chunks, k_spmv_long_finish) on the CPU emulation build of the
HIP sources, on the systems with directed row shapes of rowshape_cases.py: zk_ctx_probe_rows row by row against Python dot products, the
witness map against the oracle and pyref, proof bytes against the oracle with four and with six transforms, the refusal of a witness that
differs only in what a later chunk of a long row reads, the probe's own refusals.  rowshape_checks.py documents the checks;
test_rowshape_gpu.py runs the same ones on the device.

The probe and the witness map run on contexts made with ZK_SIX_TRANSFORMS=1: the row evaluation is one helper under both pipelines, and the
stand-in builds the four-transform tables of a system whose C has 40 000 non-zeros in 40 s.  The proofs run on both paths; those that build such
tables, or prove a domain of 512 on the stand-in, are marked slow."""
import ctypes as C
import pytest
import rowshape_cases as cases
import rowshape_checks as chk


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


@pytest.mark.parametrize("name", cases.ROW_CASES + ("late",))
def test_generated_system_reaches_its_edge_and_is_satisfied(name):
    cases.witnesses(name)                                            # asserts is_satisfied for every witness; system() asserts the shape


@pytest.mark.parametrize("name", cases.ROW_CASES)
def test_rows_are_the_dot_products(zk, oracle, name):
    chk.check_rows(zk, oracle, name, six=True)


@pytest.mark.parametrize("name", cases.ROW_CASES)
def test_rows_of_edge_witnesses_and_canonical_input(zk, oracle, name):
    chk.check_edge_witnesses(zk, oracle, name, six=True)


@pytest.mark.parametrize("name", cases.ROW_CASES)
def test_witness_map_is_the_oracles(zk, oracle, name):
    chk.check_witness_map(zk, oracle, name, six=True)


DOMAIN_512 = ("lengths_general", "padding_256_0", "padding_251_5", "padding_3_300", "padding_256_255")


def _proof_params():
    for name in cases.PROOF_CASES:
        for six in (False, True):
            slow = name in DOMAIN_512 or (not six and name == "many_long")
            yield pytest.param(name, six, marks=[pytest.mark.slow] if slow else [], id="%s-%s" % (name, "six" if six else "four"))


@pytest.mark.parametrize("name,six", list(_proof_params()))
def test_proof_bytes_are_the_oracles(zk, oracle, name, six):
    chk.check_proofs(zk, oracle, name, six)


@pytest.mark.parametrize("six", [pytest.param(False, marks=pytest.mark.slow, id="four"), pytest.param(True, id="six")])
def test_a_witness_wrong_in_a_later_chunk_is_refused(zk, oracle, six):
    chk.check_refusal(zk, oracle, six)


def test_probe_refusals(zk, oracle):
    chk.check_probe_refusals(zk, oracle, six=True)
