"""The device pairing of csrc/pairing.hpp value by value: zk_pairing_probe on the GPU -- the non-inlined tower, step and loop functions
that k_vfy_pairing calls, in the loose domain [0, 2q), also with the output aliasing an input as the pairing calls them -- against
oracle/pyref.py over the full operand lists of tests/pairing_cases.py: coefficients at q, q + 1, 2q - 1, Karatsuba sums on either
representative of zero, lines with a vanishing coefficient, every pair of representatives for the predicates; and k_vfy_prepare alone
(zk_vctx_probe_prepare) on digits at the signed-window boundary, carries through every window, an accumulator that passes through
infinity and a term equal to the accumulator.  Every raw output word is also asserted to lie in [0, 2q).  One launch per op and list;
the slow part is the Python reference.  test_pairing_emul.py pins the reference and the identities on the CPU."""
import pytest
import pairing_cases as K
import pairing_checks as chk

pytestmark = pytest.mark.gpu


def test_operand_lists_hold_the_hard_cases():
    K.premises()


def test_fq2_helpers(hip):
    chk.check_fq2_helpers(hip, loose=True)


def test_fq6(hip):
    chk.check_fq6(hip, loose=True)


def test_f12_mul_dense_aliased_and_sparse(hip):
    chk.check_f12_mul(hip, loose=True)


def test_f12_mul034(hip):
    chk.check_f12_mul034(hip, loose=True)


def test_f12_sqr_conj_canon(hip):
    chk.check_f12_sqr_conj_canon(hip, loose=True)


def test_f12_inv(hip):
    chk.check_f12_inv(hip, loose=True)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_f12_frobenius(hip, k):
    chk.check_f12_frobenius(hip, True, k)


def test_f12_predicates(hip):
    chk.check_f12_predicates(hip, loose=True)


def test_cyclotomic_square_and_exp_negz(hip):
    chk.check_cyclotomic(hip, loose=True)


def test_final_exponentiation(hip):
    chk.check_final_exp(hip, loose=True)


def test_miller_steps(hip):
    chk.check_steps(hip, loose=True)


def test_g2_frobenius(hip):
    chk.check_g2_frobenius(hip, loose=True)


def test_ell(hip):
    chk.check_ell(hip, loose=True)


def test_miller_loop_variable_multi_and_fixed(hip):
    chk.check_miller(hip, loose=True)


def test_pair_product_values(hip):
    chk.check_pair_product(hip, loose=True)


def test_point_predicates(hip):
    chk.check_point_predicates(hip, loose=True)


@pytest.mark.parametrize("tables", [True, False], ids=["window tables", "double-and-add"])
def test_prepare_kernel(hip, tables, monkeypatch):
    def make(vk_json, max_batch):
        if not tables:
            monkeypatch.setenv("ZK_VERIFY_TABLE_BUDGET", "1")
        try:
            return hip.Verifier(vk_json, max_batch=max_batch)
        finally:
            monkeypatch.delenv("ZK_VERIFY_TABLE_BUDGET", raising=False)
    chk.check_prepare(hip, make)
