"""The dedicated field squaring on the device (bn254.hpp sqr_fips / sqr_fips_x2 behind Field::lsqr / lsqr_pair): the operand list of
tests/fq_squaring_checks.py through the arithmetic probe against lmul(a, a) and big-int arithmetic, the G1 formulas that square (madd,
madd_pairs, dbl, dbl_affine, add on loose coordinates with P + P, P - P and infinity on either side) against the oracle's points, one G1
multi-exponentiation of 2^10 bases and one 2^10 proof against the oracle."""
import numpy as np
import pytest
import fq_squaring_checks as SC
from ethsnarks_amd import fields as F, r1cs as R
from helpers import rand_scalars, tiled_bases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_lsqr_on_loose_operands(hip, field):
    SC.check_lsqr(hip, field)


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_lsqr_pair_is_two_lsqr(hip, field):
    SC.check_lsqr_pair(hip, field)


@pytest.mark.parametrize("name", SC.G1_FORMULAS)
def test_g1_formula_against_the_oracle(hip, oracle, name):
    SC.check_g1_formula(hip, oracle, name, loose=True)


def test_g1_msm_1024_bases(hip, oracle):
    n = 1 << 10
    sc = rand_scalars(n, 78, ones_every=5, zeros_every=7)
    sc[11] = F.FR - 1; sc[12] = 2; sc[13] = 1 << 253
    s = F.fr_to_mont(sc)
    bases = tiled_bases(oracle, n, g2=False, distinct=512)
    bases[20] = 0; bases[21] = bases[22]
    assert np.array_equal(hip.msm(bases, s, g2=False), oracle.msm(bases, s, g2=False))


def test_proof_of_1024_constraints_is_the_oracles(hip, oracle):
    r, w = R.synthetic_chain((1 << 10) - 2, 1)
    wm = F.fr_to_mont(w)
    pk_o, _ = oracle.keygen(r, seed=1)
    expect, _ = oracle.prove(pk_o, r, wm)
    pk = hip.ProvingKey.from_parts(**pk_o.parts())
    assert hip.prove(hip.ProverContext(pk, r), wm) == expect
