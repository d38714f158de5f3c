"""What test_merkle_update_emul.py and test_merkle_update_gpu.py share: MerkleTree.update_seq (zk_mtree_update_seq) against the references of
merkle_update_cases.py -- the PyTree chain for roots and nodes, the witness of gadgets.merkle_update_circuit and inputs + WitnessPlan.solve for
the rows.  Every comparison is exact: ints, or np.array_equal on limbs."""
import os

import numpy as np
import pytest
from ethsnarks_amd import fields as F
import merkle_update_cases as UC
from full_witness_checks import sentinel, check_proof  # noqa: F401

FR_LIMBS = F.ints_to_limbs([F.FR])                                # the modulus itself as "canonical" limbs: a leaf that is not below r


def new_tree(M, hasher, case, no_tail=False):
    """the device tree of a case; no_tail: every level of every hashing phase gets its own launch (ZK_MTREE_NO_TAIL at creation)"""
    if no_tail:
        os.environ["ZK_MTREE_NO_TAIL"] = "1"
    try:
        t = M.MerkleTree(1 << case.depth, hasher=hasher)
    finally:
        os.environ.pop("ZK_MTREE_NO_TAIL", None)
    t.extend(case.leaves)
    return t


def run(zk, M, hasher, case, elems, no_tail=False, **kw):
    """(tree after, roots, sentinel, buffer after update_seq) with k + 1 rows of `elems` elements"""
    k = len(case.indices)
    t = new_tree(M, hasher, case, no_tail)
    s = sentinel(k + 1, elems)
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    roots = t.update_seq(case.indices, case.values, buf, row_elems=elems, **kw)
    got = buf.download(s.shape)
    buf.free()
    return t, roots, s, got


def solved_rows(zk, r, hasher, D, ref, extra_rows=1):
    """the same rows by the planner: a sentinel buffer that holds only the inputs (from the PyTree chain), then WitnessPlan.solve"""
    k, n_in = len(ref.inputs), UC.n_supplied(hasher, D)
    s = sentinel(k + extra_rows, r.V + 1)
    for j, row in enumerate(ref.inputs):
        s[j, :n_in] = F.fr_to_mont(row)
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    plan = zk.WitnessPlan(r, list(range(n_in)))
    assert plan.solve(buf.ptr, k) == 0
    got = buf.download(s.shape)
    plan.close(); buf.free()
    return got


def check_case(zk, M, hasher, case, ref, r, rows=None, no_tail=False):
    """rows against the gadgets' witnesses (all of ref.circuits, or `rows`), the row after the last and the roots inside the rows, the root chain
    and every node against the PyTree.  Returns (tree, roots, rows)"""
    k, D = len(case.indices), case.depth
    layout, var0, stride, elems = M.update_layout(D, hasher)
    assert (var0, stride, elems) == (UC.n_supplied(hasher, D), UC.STRIDE[hasher], r.V + 1)
    t, roots, s, got = run(zk, M, hasher, case, elems, no_tail)
    assert roots == ref.roots
    for j in (sorted(ref.circuits) if rows is None else rows):
        assert np.array_equal(got[j], F.fr_to_mont(ref.circuits[j][1])), (hasher, k, j)
    assert np.array_equal(got[k], s[k])
    for j in range(k):                                             # every row's two roots, also where no gadget witness was built
        assert np.array_equal(got[j, 1:3], F.fr_to_mont(roots[j:j + 2])), (hasher, k, j)
    UC.assert_same_nodes(hasher, t, ref.tree)
    return t, roots, got


def check_tail_untouched(zk, M, hasher, case, r, got, tail=5):
    """a longer row_elems: the same rows, and the tail of every row keeps the sentinel"""
    k = len(case.indices)
    t, _, s2, got2 = run(zk, M, hasher, case, r.V + 1 + tail)
    assert np.array_equal(got2[:k, :r.V + 1], got[:k]) and np.array_equal(got2[:, r.V + 1:], s2[:, r.V + 1:]) and np.array_equal(got2[k], s2[k])
    t.close()


def check_single_updates_agree(M, hasher, case, ref):
    """a second device tree given the same updates by k single update() calls, and a third by update_seq without a buffer: same roots and nodes"""
    t2 = new_tree(M, hasher, case)
    for a, y in zip(case.indices, case.values):
        t2.update(a, y)
    UC.assert_same_nodes(hasher, t2, ref.tree)
    t3 = new_tree(M, hasher, case)
    assert t3.update_seq(case.indices, case.values) == ref.roots
    UC.assert_same_nodes(hasher, t3, ref.tree)
    for d in range(case.depth + 1):
        for o in range(len(ref.tree.levels[d])):
            assert t2.leaf(d, o) == t3.leaf(d, o)
    t2.close(); t3.close()


def check_refusals(zk, M, hasher, case):
    """every bad call is ZK_ERR_ARG with a message, and leaves the root, every node and the buffer as they were; k = 0 returns [root]"""
    D = case.depth
    ref = UC.ref_tree(hasher, D, case.leaves)
    t = new_tree(M, hasher, case)
    L, var0, stride, elems = M.update_layout(D, hasher)
    mk = lambda **kw: M.UpdateLayout(*[kw.get(n, getattr(L, n)) for n, _ in M.UpdateLayout._fields_])
    n = len(case.leaves)
    good = F.ints_to_limbs([5])

    def refused(tree, indices, leaves, layout=L, row_elems=elems, level_var0=var0, level_stride=stride, tree_ref=ref):
        s = sentinel(2, elems + 8)
        buf = zk.DeviceBuffer(s.nbytes)
        buf.upload(s)
        for target in (buf.ptr, None):                             # with and without a witness buffer (the layout is not read without one)
            if target is None and (layout is not L or (row_elems, level_var0, level_stride) != (elems, var0, stride)):
                continue
            with pytest.raises(zk.ZkError) as e:
                tree.update_seq(indices, leaves, target, layout, row_elems=row_elems, level_var0=level_var0, level_stride=level_stride)
            assert e.value.code == 1 and zk._lib.zk_last_error() and len(str(e.value)) > len("zkhip error 1: ")
            assert np.array_equal(buf.download(s.shape), s)
            if tree_ref is not None:
                UC.assert_same_nodes(hasher, tree, tree_ref)
        buf.free()

    refused(t, [n], good)                                          # an index equal to the size
    refused(t, [0, n], np.concatenate([good, good]))               # ... after a good one: nothing of the call is applied
    refused(t, [1], FR_LIMBS)                                      # a leaf equal to r
    refused(t, [0, 1], np.concatenate([good, FR_LIMBS]))
    refused(t, [0], good, level_stride=stride - 1)                 # level_stride one short
    refused(t, [0], good, layout=mk(new_leaf_var=var0 + 5))        # a level block overlapping new_leaf_var
    refused(t, [0], good, layout=mk(new_leaf_var=var0 + 2 * D * stride - 1))               # ... the last element of the new chain's blocks
    refused(t, [0], good, row_elems=elems - 1)                     # row_elems one short: the last block leaves the row
    refused(t, [0], good, layout=mk(old_root_var=elems), row_elems=elems)                  # an input outside the row
    if hasher == "poseidon":
        refused(t, [0], good, layout=mk(iv_var0=elems, n_iv=29), row_elems=elems + 29)     # n_iv = 29 on Poseidon
    else:
        refused(t, [0], good, layout=mk(n_iv=D - 1))              # n_iv = D - 1 on MiMC: the IVs of every level are read
    empty = M.MerkleTree(1 << D, hasher=hasher)
    refused(empty, [0], good, tree_ref=None)                       # an empty tree
    assert len(empty) == 0 and empty.root is None
    with pytest.raises(zk.ZkError):
        empty.update_seq([], [])                                   # ... has no root to return either
    # k = 0: [root], nothing written
    s = sentinel(1, elems)
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    assert t.update_seq([], [], buf, L, row_elems=elems) == [ref.root] and t.update_seq([], []) == [ref.root]
    assert np.array_equal(buf.download(s.shape), s)
    UC.assert_same_nodes(hasher, t, ref)
    with pytest.raises(ValueError):
        t.update_seq([0, 1], [1, 2], buf, L, row_elems=elems)      # the buffer holds one row
    with pytest.raises(ValueError):
        t.update_seq([0, 1], [1])
    buf.free(); empty.close(); t.close()


def check_wide_tree_refused(zk, M, D=3):
    t = M.MerkleTree(4 ** D, width=4, hasher="poseidon")
    t.extend([1, 2, 3, 4, 5])
    root = t.root
    L, var0, stride, elems = M.update_layout(D, "poseidon")
    s = sentinel(1, elems)
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    for target in (buf, None):
        with pytest.raises(zk.ZkError) as e:
            t.update_seq([0], [7], target, L, row_elems=elems)
        assert e.value.code == 1
    assert np.array_equal(buf.download(s.shape), s) and t.root == root and [t[i] for i in range(5)] == [1, 2, 3, 4, 5]
    buf.free(); t.close()
