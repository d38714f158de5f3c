"""The pairing probe (zk_pairing_probe, zk_vctx_probe_prepare) in the CPU emulation build of csrc/verify_gpu.cpp against oracle/pyref.py,
over the canonical half of the operand lists (tests/pairing_cases.py, loose=False: in this build the loose names are the strict host
operations, and values at or above q are outside their contract).  This file pins the reference, the word layouts and the identities the
device tests rely on -- the Miller value against pyref after the easy part of the final exponentiation, the products of single-pair
values, the fixed-Q route -- where they can run without a GPU.  test_pairing_gpu.py runs the full lists through the device tower.

The premise assertions of the operand lists need no library at all and run here as well."""
import numpy as np
import pytest
import pairing_cases as K
import pairing_checks as chk
from test_verify_batch_emul import emul_verify, zk        # noqa: F401  (the fixtures of the verifier's emulation library)


def test_operand_lists_hold_the_hard_cases():
    K.premises()


def test_fq2_helpers(zk):
    chk.check_fq2_helpers(zk, loose=False)


def test_fq6(zk):
    chk.check_fq6(zk, loose=False)


def test_f12_mul_dense_aliased_and_sparse(zk):
    chk.check_f12_mul(zk, loose=False)


def test_f12_mul034(zk):
    chk.check_f12_mul034(zk, loose=False)


def test_f12_sqr_conj_canon(zk):
    chk.check_f12_sqr_conj_canon(zk, loose=False)


def test_f12_inv(zk):
    chk.check_f12_inv(zk, loose=False)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_f12_frobenius(zk, k):
    chk.check_f12_frobenius(zk, False, k)


def test_f12_predicates(zk):
    chk.check_f12_predicates(zk, loose=False)


def test_cyclotomic_square_and_exp_negz(zk):
    chk.check_cyclotomic(zk, loose=False)


def test_final_exponentiation(zk):
    chk.check_final_exp(zk, loose=False)


def test_miller_steps(zk):
    chk.check_steps(zk, loose=False)


def test_g2_frobenius(zk):
    chk.check_g2_frobenius(zk, loose=False)


def test_ell(zk):
    chk.check_ell(zk, loose=False)


def test_miller_loop_variable_multi_and_fixed(zk):
    chk.check_miller(zk, loose=False)


def test_pair_product_values(zk):
    chk.check_pair_product(zk, loose=False)


def test_point_predicates(zk):
    chk.check_point_predicates(zk, loose=False)


@pytest.mark.parametrize("tables", [True, False], ids=["window tables", "double-and-add"])
def test_prepare_kernel(zk, tables, monkeypatch):
    def make(vk_json, max_batch):
        if not tables:
            monkeypatch.setenv("ZK_VERIFY_TABLE_BUDGET", "1")
        try:
            return zk.Verifier(vk_json, max_batch=max_batch)
        finally:
            monkeypatch.delenv("ZK_VERIFY_TABLE_BUDGET", raising=False)
    chk.check_prepare(zk, make)


def test_probe_argument_checks(zk):
    """the ABI's rules: unknown ops and null buffers are ZK_ERR_ARG, zero cases are fine"""
    for op in (-1, 46, 0x100):
        with pytest.raises(zk.ZkError) as e:
            zk.pairing_probe_shape(op)
        assert e.value.code == 1
        assert zk._lib.zk_pairing_probe(op, None, 0, None, 0) == 1
    assert sorted(K.OPS.values()) == list(range(46)) and set(K.OPS) == set(K.SHAPES)
    for name, op in K.OPS.items():
        assert zk.pairing_probe_shape(op) == K.SHAPES[name], name
    assert zk._lib.zk_pairing_probe(0, None, 3, None, 0) == 1
    assert zk._lib.zk_pairing_probe(0, None, (1 << 12) + 1, None, 0) == 1
    assert zk.pairing_probe(0, np.zeros((0, 12, 4), dtype=np.uint64)).shape == (0, 6, 4)
    assert zk._lib.zk_vctx_probe_prepare(None, None, None, 1, None) == 1
