"""The arithmetic probe (zk_arith_probe) in the CPU emulation build against tests/arith_ref.py, over the canonical half of the operand
lists (tests/arith_cases.py, loose=False): in this build the loose names are the strict host operations, the _q forms the plain ones
and the product pairs two single products, so this file pins the host half of csrc/bn254.hpp and the probe's own plumbing.  The
gfx950 assembly layer -- the loose domain itself -- is what test_arith_gpu.py runs the full lists through.

The premise assertions of the operand lists need no library at all and run here as well."""
import numpy as np
import pytest
import arith_cases as K
import arith_checks as chk
import arith_ref as A


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


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_operand_lists_hold_the_hard_cases(field):
    """from the reference alone: both fold classes of lmul2, all three of lmul4, the differences 0 / p / 2p - 1, sums in [2p, 4p), the
    near misses of lis_zero -- and every operand inside its primitive's contract"""
    K.premises(A.MOD[field])


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_reference_agrees_with_the_oracle_products(oracle, field):
    chk.check_reference_against_oracle(oracle, field)


@pytest.mark.parametrize("field", ["fr", "fq"])
@pytest.mark.parametrize("name", list(K.FIELD_OPS))
def test_field_op(zk, field, name):
    chk.check_field_op(zk, field, name, loose=False)


@pytest.mark.parametrize("field", ["fr", "fq"])
@pytest.mark.parametrize("name", ["lmul_x2", "lmul2_x2"])
def test_product_pairs_equal_single_products(zk, field, name):
    chk.check_field_x2(zk, field, name, loose=False)


@pytest.mark.parametrize("name", list(K.FQ2_OPS))
def test_fq2_op(zk, name):
    chk.check_fq2_op(zk, name, loose=False)


@pytest.mark.parametrize("g2", [False, True], ids=["G1", "G2"])
@pytest.mark.parametrize("name", list(K.CURVE_OPS))
def test_curve_op(zk, oracle, g2, name):
    chk.check_curve_op(zk, oracle, g2, name, loose=False)


def test_probe_argument_checks(zk):
    """the ABI's rules: unknown ops and null buffers are ZK_ERR_ARG, zero cases are fine"""
    for op in (-1, 24, zk.PROBE_FQ + 24, zk.PROBE_FQ2 + 11, zk.PROBE_G1 + 10, zk.PROBE_G2 + 10, 0x500):
        with pytest.raises(zk.ZkError) as e:
            zk.arith_probe_shape(op)
        assert e.value.code == 1
        assert zk._lib.zk_arith_probe(op, None, 0, None, 0) == 1
    assert zk._lib.zk_arith_probe(zk.PROBE_FR, None, 3, None, 0) == 1
    assert zk._lib.zk_arith_probe(zk.PROBE_FR, None, (1 << 20) + 1, None, 0) == 1
    assert zk.arith_probe(zk.PROBE_FR, np.zeros((0, 2, 4), dtype=np.uint64)).shape == (0, 1, 4)
