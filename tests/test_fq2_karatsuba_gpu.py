"""The lazy Karatsuba Fq2 product on the device (fips_asm.hpp karat_comb8_*, bn254.hpp Field::lmul_k / lmul2_k): the operand lists of
tests/fq2_karatsuba_checks.py through the arithmetic probe, the G2 formulas that are made of it (madd, dbl, dbl_affine on loose coordinates
with every exceptional case: P + P, P - P, infinity on either side) against the reference, one G2 multi-exponentiation of 2^10 bases
and one 2^10 proof against the oracle."""
import numpy as np
import pytest
import arith_checks as chk
import fq2_karatsuba_checks as KC
from ethsnarks_amd import fields as F, r1cs as R
from helpers import rand_scalars, tiled_bases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["lmul", "lmul2"])
def test_fq2_product_on_loose_operands(hip, name):
    KC.check(hip, name)


@pytest.mark.parametrize("name", ["madd", "dbl", "dbl_affine"])
def test_g2_formula(hip, oracle, name):
    chk.check_curve_op(hip, oracle, True, name, loose=True)


def test_g2_msm_1024_bases(hip, oracle):
    n = 1 << 10
    sc = rand_scalars(n, 77, ones_every=5, zeros_every=7)
    sc[11] = F.FR - 1; sc[12] = 2; sc[13] = 1 << 253
    s = F.fr_to_mont(sc)
    bases = tiled_bases(oracle, n, g2=True, distinct=512)
    bases[20] = 0; bases[21] = bases[22]
    assert np.array_equal(hip.msm(bases, s, g2=True), oracle.msm(bases, s, g2=True))


def test_proof_of_1024_constraints_is_the_oracles(hip, oracle):
    r, w = R.synthetic_chain((1 << 10) - 2, 1)
    wm = F.fr_to_mont(w)
    pk_o, _ = oracle.keygen(r, seed=1)
    expect, _ = oracle.prove(pk_o, r, wm)
    pk = hip.ProvingKey.from_parts(**pk_o.parts())
    assert hip.prove(hip.ProverContext(pk, r), wm) == expect
