"""MerkleTree.fill_full_witnesses (zk_mtree_fill_full_witnesses; k_mtree_fill_levels of csrc/merkle.hpp, permute_traced of csrc/poseidon.hpp) on the
CPU emulation build: the complete membership witness straight from the tree, for both hashers, against the witness of the Python gadgets and
against fill_witnesses + WitnessPlan.solve.  Everything is integer arithmetic and compares byte for byte.  test_full_witness_gpu.py runs the same
checks on the device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import merkle_cases as MC
import full_witness_checks as chk
from full_witness_checks import HASHERS


@pytest.fixture(scope="module")
def emul_merkle(emul):
    from conftest import ROOT
    d = os.path.join(ROOT, "tests", "emul_merkle")
    so = os.path.join(d, "libzkhip_emul_merkle.so")
    csrc = os.path.join(ROOT, "ethsnarks_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith("pp")] + [emul, os.path.join(d, "Makefile")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", d, "-s"])
    return so


@pytest.fixture(scope="module")
def zk(emul_merkle):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul_merkle)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    prover._lib = None
    prover._lib_path_loaded = None


@pytest.fixture(scope="module")
def M(zk):
    from ethsnarks_amd import merkle
    return merkle


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


D = 3


@pytest.fixture(scope="module")
def depth3(zk, M):
    """per hasher: the tree of 7 leaves, its constraint system, the witnesses of indices [0, 6, 3] and the rows fill_full_witnesses wrote"""
    out = {}
    for hasher in HASHERS:
        out[hasher] = chk.check_rows_against_gadgets(zk, M, hasher, D, 7, [0, 6, 3], 960)      # 6: placeholders on its path
    yield out
    for t, _, _, _ in out.values():
        t.close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_rows_equal_the_gadgets_witness(zk, M, depth3, hasher):
    assert hasher in depth3                                        # n = 7, indices [0, 6, 3]: checked by the fixture
    ref = chk.ref_tree(hasher, D, MC.random_leaves(7, 960))
    assert (ref.placeholder_levels(6) if hasher == "mimc" else ref.placeholders(6))
    t = chk.check_rows_against_gadgets(zk, M, hasher, D, 8, [7], 961)[0]      # a full tree; every bit of 7 selects the right side
    t.close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_same_bytes_as_fill_witnesses_and_solve(zk, depth3, hasher):
    t, r, _, got = depth3[hasher]
    assert np.array_equal(chk.solved(zk, t, [0, 6, 3], r, hasher), got)


@pytest.mark.parametrize("hasher", HASHERS)
def test_one_row_proves(zk, oracle, depth3, hasher):
    _, r, cases, got = depth3[hasher]
    chk.check_proof(zk, oracle, r, cases[1][1], got[1])


@pytest.mark.parametrize("hasher", HASHERS)
def test_repeated_indices(zk, depth3, hasher):
    t, r, cases, got = depth3[hasher]
    _, two = chk.filled(zk, t, [3, 3], r)
    assert np.array_equal(two[0], two[1]) and np.array_equal(two[0], got[2])


@pytest.mark.parametrize("hasher", HASHERS)
def test_explicit_layout_places_the_level_blocks(zk, M, depth3, hasher):
    """inputs and level blocks away from the allocation order, a stride above the level's variables, three IVs instead of 29: every block is
    where the arguments put it and everything between and after the blocks keeps the sentinel"""
    t, r, cases, _ = depth3[hasher]
    n_iv = D if hasher == "mimc" else 0
    L = M.Layout(4, 10, 20, 2, 30 if n_iv else 0, n_iv)
    var0, stride, size = 41, chk.STRIDE[hasher] + 9, chk.STRIDE[hasher]
    elems = var0 + D * stride + 3
    s, got = chk.filled(zk, t, [6, 0], L, row_elems=elems, level_var0=var0, level_stride=stride)
    src0 = chk.n_supplied(hasher, D)                                # the first level variable in the allocation order
    for p, c in enumerate((cases[1], cases[0])):
        w = F.fr_to_mont(c[1])
        want = s[p].copy()
        want[0] = w[0]; want[4] = w[1]; want[10:10 + D] = w[2:2 + D]; want[20:20 + D] = w[2 + D:2 + 2 * D]; want[2] = w[2 + 2 * D]
        want[30:30 + n_iv] = w[3 + 2 * D:3 + 2 * D + n_iv]
        for d in range(D):
            want[var0 + d * stride:var0 + d * stride + size] = w[src0 + d * size:src0 + (d + 1) * size]
        assert np.array_equal(got[p], want), (hasher, p)
    assert np.array_equal(got[2], s[2])


def refused(zk, M, t, hasher, indices, layout, elems, var0, stride):
    """ZK_ERR_ARG, a message, and the buffer as it was"""
    s = chk.sentinel(2, elems)
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    with pytest.raises(zk.ZkError) as e:
        t.fill_full_witnesses(indices, buf.ptr, layout, row_elems=elems, level_var0=var0, level_stride=stride)
    assert e.value.code == 1 and zk._lib.zk_last_error() and len(str(e.value)) > len("zkhip error 1: ")
    assert np.array_equal(buf.download(s.shape), s)
    buf.free()


@pytest.mark.parametrize("hasher", HASHERS)
def test_bad_arguments_are_refused(zk, M, depth3, hasher):
    t = depth3[hasher][0]
    L, var0, stride, elems = M.membership_full_layout(D, hasher)
    mk = lambda **kw: M.Layout(*[kw.get(n, getattr(L, n)) for n, _ in M.Layout._fields_])
    bad = [([7], L, elems, var0, stride),                           # an index >= the size
           ([0, 7], L, elems, var0, stride),
           ([0], L, elems, var0, stride - 1),                       # a stride below the variables of a level
           ([0], L, elems - 1, var0, stride),                       # the last level block leaves the row
           ([0], L, elems, var0 + 1, stride),
           ([0], mk(root_var=elems), elems, var0, stride),          # the layout leaves the row
           ([0], mk(path_var0=elems - D + 1), elems, var0, stride),
           ([0], L, elems + stride, var0 - 1, stride),              # the level blocks overlap the last input variable ...
           ([0], mk(leaf_var=var0 + 5), elems, var0, stride),       # ... the leaf ...
           ([0], mk(root_var=var0 + D * stride - 1), elems, var0, stride),
           ([0], mk(addr_var0=var0 - 1), elems, var0, stride),      # ... the address bits
           ([0], L, elems, 0, stride)]                              # ... ONE
    if hasher == "poseidon":
        bad.append(([0], mk(iv_var0=elems + 1, n_iv=1), elems + 8, var0, stride))            # Poseidon has no IVs
    else:
        bad.append(([0], mk(n_iv=D - 1), elems, var0, stride))      # the IVs of every level are read
        bad.append(([0], mk(n_iv=30), elems, var0, stride))
        bad.append(([0], mk(iv_var0=var0 + 2), elems + 40, var0, stride))
    for case in bad:
        refused(zk, M, t, hasher, *case)
    empty = M.MerkleTree(1 << D, hasher=hasher)
    refused(zk, M, empty, hasher, [0], L, elems, var0, stride)
    # k = 0: nothing happens, on a tree with leaves and on an empty one
    s = chk.sentinel(1, elems)
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    t.fill_full_witnesses([], buf, L, row_elems=elems)
    empty.fill_full_witnesses([], buf, L, row_elems=elems)
    assert np.array_equal(buf.download(s.shape), s)
    with pytest.raises(ValueError):
        t.fill_full_witnesses([0, 1], buf, L, row_elems=elems)      # the buffer holds one row
    buf.free(); empty.close()


def test_wide_poseidon_trees_are_refused(zk, M):
    for width in (3, 4):
        t = M.MerkleTree(width ** D, width=width, hasher="poseidon")
        t.extend([1, 2, 3, 4])
        L, var0, stride, elems = M.membership_full_layout(D, "poseidon")
        refused(zk, M, t, "poseidon", [0], L, elems, var0, stride)
        t.close()
