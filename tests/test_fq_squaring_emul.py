"""The dedicated field squaring in the CPU emulation build: Field::lsqr (sqr_cols_c, the device's column form step for step in plain C++)
and lsqr_pair through the arithmetic probe against lmul(a, a) and big-int arithmetic on LOOSE operands up to 2p - 1, and the G1 formulas
that square (madd, madd_pairs, dbl, dbl_affine, add) against the oracle's points.  Lists and contracts: tests/fq_squaring_checks.py."""
import pytest
import fq_squaring_checks as SC


@pytest.fixture(scope="module")
def zk(emul):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    prover._lib = None
    prover._lib_path_loaded = None


def test_operand_lists_hold_the_named_cases():
    SC.premises()


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_lsqr_on_loose_operands(zk, field):
    SC.check_lsqr(zk, field)


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_lsqr_pair_is_two_lsqr(zk, field):
    SC.check_lsqr_pair(zk, field)


@pytest.mark.parametrize("name", SC.G1_FORMULAS)
def test_g1_formula_against_the_oracle(zk, oracle, name):
    SC.check_g1_formula(zk, oracle, name, loose=False)
