"""The gfx950 assembly layer of csrc/bn254.hpp (fips_asm.hpp: the loose domain [0, 2p)) primitive by primitive: zk_arith_probe on the
device against tests/arith_ref.py over the full operand lists of tests/arith_cases.py -- operands at 2p - 1 and 2p, sums that need the
second fold, differences that land on the representative p of zero, limbs of all ones -- plus the curve formulas on loose coordinates
and every exceptional case, the quad forms on four lanes, and the same lists through the build without the assembly post-pass."""
import os
import subprocess
import sys
import numpy as np
import pytest
import arith_cases as K
import arith_checks as chk
import arith_ref as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_operand_lists_hold_the_hard_cases(field):
    K.premises(A.MOD[field])


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_reference_agrees_with_the_oracle_products(oracle, field):
    chk.check_reference_against_oracle(oracle, field)


@pytest.mark.parametrize("field", ["fr", "fq"])
@pytest.mark.parametrize("name", list(K.FIELD_OPS))
def test_field_op(hip, field, name):
    chk.check_field_op(hip, field, name, loose=True)


@pytest.mark.parametrize("field", ["fr", "fq"])
@pytest.mark.parametrize("name", ["lmul_x2", "lmul2_x2"])
def test_product_pairs_equal_single_products(hip, field, name):
    chk.check_field_x2(hip, field, name, loose=True)


@pytest.mark.parametrize("name", list(K.FQ2_OPS))
def test_fq2_op(hip, name):
    chk.check_fq2_op(hip, name, loose=True)


@pytest.mark.parametrize("g2", [False, True], ids=["G1", "G2"])
@pytest.mark.parametrize("name", list(K.CURVE_OPS))
def test_curve_op(hip, oracle, g2, name):
    chk.check_curve_op(hip, oracle, g2, name, loose=True)


def test_probe_without_the_assembly_postpass_gives_identical_raw_results(hip, oracle, tmp_path):
    """the whole field and curve case list through variants/nopostpass/libzkhip.so (the same sources built with POSTPASS=0, made by
    __graft_entry__.build()) in a child process: the raw outputs are those of the default build, limb for limb"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "variants", "nopostpass", "libzkhip.so")
    assert os.path.exists(so), "variants/nopostpass/libzkhip.so missing: run __graft_entry__.build()"
    npz = str(tmp_path / "nopostpass.npz")
    code = '''
import sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import oracle_lib as O
import arith_checks as chk
from ethsnarks_amd import prover as P
P.load_library(%r)
np.savez(%r, **chk.all_raw_outputs(P, O, True))
print("DONE")
''' % (root, os.path.join(root, "tests"), os.path.join(root, "oracle"), so, npz)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "DONE" in p.stdout, p.stderr[-2000:]
    other = np.load(npz)
    mine = chk.all_raw_outputs(hip, oracle, True)
    assert sorted(other.files) == sorted(mine)
    for key in sorted(mine):
        a, b = mine[key], other[key]
        assert a.shape == b.shape, key
        rows = np.nonzero((a != b).any(axis=1))[0]
        assert rows.size == 0, "%s: result word %d differs between the builds: %s (default) against %s (no post-pass)" % (
            key, rows[0], [hex(int(v)) for v in a[rows[0]]], [hex(int(v)) for v in b[rows[0]]])
