"""The witness fill of the EdDSA circuit of the "hash" scheme on the CPU emulation build of the HIP sources (csrc/jubjub.hpp k_eddsa_fill_hash,
jubjub.cpp): rows against the front end's generate_r1cs_witness element by element at n = 1, 3 and 65; the shapes of the message hash -- no
padding bit (the reference's own signature), another base point, a second segment with its Edwards adder, a lone last window -- verdicts,
sentinels, refusals, the front end's layout and its rejection of a non-canonical decomposition of M.x, and one chain from the signer through the
circuit's keygen to a verified proof.  test_eddsa_hash_gpu.py runs the same checks on the device.  One lane writes one row and no lanes
cooperate, so the emulator's lane order does not enter."""
import ctypes as C

import pytest

from ethsnarks_amd import jubjub_gadgets as JG
from ethsnarks_amd.fields import FR
import eddsa_hash_cases as HC
import eddsa_hash_checks as chk
import jubjub_cases as JC
from test_jubjub_emul import emul_jubjub, zk, J                        # noqa: F401  (the fixtures that build and load the emulation library)


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


@pytest.mark.parametrize("n", HC.SIZES)
def test_rows_and_verdicts(zk, J, n):
    chk.check_rows(zk, J, n)


def test_no_padding_bit_reference_signature(zk, J):
    chk.check_items(zk, J, [HC.reference_signature()], 3)


def test_two_padding_bits_and_another_base_point(zk, J):
    B = JC.mul(JC.GENERATOR, 77)
    chk.check_items(zk, J, [HC.one_valid(2, B)], 2, B)


def test_second_segment_and_edwards_adder(zk, J):
    chk.check_items(zk, J, [HC.one_valid(HC.TWO_SEGMENT_MSG_LEN)], HC.TWO_SEGMENT_MSG_LEN)


def test_lone_last_window(zk, J):
    chk.check_items(zk, J, [HC.one_valid(HC.LONE_MSG_LEN)], HC.LONE_MSG_LEN)


@pytest.mark.parametrize("msg_len, pad, segments, lone", [(1, 1, 1, False), (2, 2, 1, False), (3, 0, 1, False), (24, 0, 2, False), (70, 1, 4, True)])
def test_layout_of_the_message_hash(J, msg_len, pad, segments, lone):
    chk.check_layout_shape(J, msg_len, pad, segments, lone)


def test_constraint_system_is_unchanged():
    """the layout is read off the allocation; not a row or a variable moves"""
    c = JG.EddsaHashCircuit(3)
    assert (c.r1cs().V, c.r1cs().nC) == (10016, 10637) == (c.layout.n_vars, c.pb.num_constraints())
    assert JG.HASH_LAYOUT_FIELDS[:25] == tuple(f for f in JG.PURE_LAYOUT_FIELDS if f != "pad_bit0") and len(JG.HASH_LAYOUT_FIELDS) == 32
    assert [n for n, _ in __import__("ethsnarks_amd.jubjub", fromlist=["x"]).EddsaHashLayout._fields_] == list(JG.HASH_LAYOUT_FIELDS)


def test_non_canonical_bits_of_the_message_hash_are_rejected():
    """front end only: the bits of M.x + r, and a signature made over THOSE bits.  Every constraint the reference has holds -- its field2bits_strict
    pins the bits up to a multiple of r, so it takes a second signature of the message -- and only the added BitsNotAbove(bits of M.x) fails"""
    A, (R, s), msg, mx = HC.non_canonical_forgery()
    c = JG.EddsaHashCircuit(1)
    c.assign(A, R, s, msg, bits_value={"m": mx + FR})
    assert [c.pb.val(b) for b in c.msg_hashed.result()] == [((mx + FR) >> i) & 1 for i in range(254)] and c.equation_holds()
    dot = lambda lc: sum(k * c.pb.values[i] for i, k in lc.items()) % FR
    bad = [i for i in range(c.pb.num_constraints()) if dot(c.pb.A[i]) * dot(c.pb.B[i]) % FR != dot(c.pb.C[i])]
    first_range = 254 + 8 + 1 + 3 * 2 + 2 * 3 + 2 + 762               # bits of s and of the message, the padding bit, the message hash, its decomposition
    assert bad and all(first_range <= i < first_range + 253 for i in bad)
    c.assign(A, R, s, msg)                                             # with the canonical bits the forged s is simply wrong
    assert not c.equation_holds() and not c.pb.is_satisfied()


def test_refusals(zk, J):
    chk.check_refusals(zk, J)


def test_one_shot_iterables(zk, J):
    chk.check_one_shot_iterables(J)


@pytest.mark.slow
def test_signed_row_proves(zk, J):
    """the whole circuit, the smallest batch: one signature of EdDSASigner("hash") becomes a proof that verifies with A and the message bits as inputs"""
    vk, texts = chk.check_proofs(zk, J, chk.signed_items(J)[:1], [True])
    assert zk.stub_verify(vk.to_json(), texts[0])
