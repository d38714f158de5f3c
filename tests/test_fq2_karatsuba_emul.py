"""The lazy Karatsuba Fq2 product in the CPU emulation build: Fq2::lmul and lmul2 through the arithmetic probe against big-int arithmetic
(tests/arith_ref.py over oracle/pyref.py) on LOOSE operands -- the portable form of Field::lmul_k computes the device algorithm step for
step (unreduced 16-limb products, the wrapped difference with its masked addition, the complemented sum), so its bounds are exercised
here up to 2q - 1 in every input.  Lists and contract: tests/fq2_karatsuba_checks.py."""
import pytest
import fq2_karatsuba_checks as KC


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


def test_operand_lists_reach_every_input_and_both_extremes():
    KC.premises()


@pytest.mark.parametrize("name", ["lmul", "lmul2"])
def test_fq2_product_on_loose_operands(zk, name):
    KC.check(zk, name)
