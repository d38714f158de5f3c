"""The device MiMC Merkle tree (zk_mtree_*, csrc/merkle.hpp + merkle.cpp, ethsnarks_amd/merkle.py) on the CPU emulation build of the HIP
sources, against the reference's known answers and a plain Python tree over gadgets.mimc_hash (merkle_cases.py).  test_merkle_gpu.py
runs the same checks and the resident proving chain on the device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F, r1cs as R
import merkle_cases as MC


@pytest.fixture(scope="module")
def emul_merkle(emul):
    """the tree's unit of the CPU emulation build (tests/emul_merkle): a library of its own beside libzkhip_emul.so, which it depends on"""
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
    """no kernel or host path of the test wrote past the end of a device buffer (tests/emul/hip_emul.h)"""
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


# ---------------------------------------------------------------- 1, 2: constants and the hash
def test_constants_equal_the_gadgets(M):
    rc, iv = M.mimc_constants()
    assert rc == G.mimc_constants()
    assert iv == G.merkle_ivs(29)


def test_mimc_hash2_against_gadgets(M):
    rng = R.SplitMix64(77)
    edge = [0, 1, F.FR - 1]
    trip = [(a, b, c) for a in edge for b in edge for c in edge] + [(rng.fr(), rng.fr(), rng.fr()) for _ in range(300)]
    trip += [(1, 1, 0)]
    got = M.mimc_hash2([t[0] for t in trip], [t[1] for t in trip], [t[2] for t in trip])
    assert got == [G.mimc_hash([a, b], c) for a, b, c in trip]
    # the reference's vectors (test/test_mimc.py; the values tests/test_gadgets.py pins gadgets.py to)
    assert got[-1] == G.mimc_hash([1, 1]) == 4087330248547221366577133490880315793780387749595119806283278576811074525767
    assert M.mimc_hash2([MC.ITEM_A], [MC.ITEM_B], [918403109389145570117360101535982733651217667914747213867238065296420114726]) == \
        [15683951496311901749339509118960676303290224812129752890706581988986633412003]


def test_mimc_hash2_rejects_operands_not_below_r(zk, M):
    with pytest.raises(zk.ZkError) as e:
        M.mimc_hash2([F.FR], [1], [0])
    assert e.value.code == 1


# ---------------------------------------------------------------- 3: the reference's known answers
def test_known1(M):
    t = M.MerkleTree(2)
    assert t.root is None and len(t) == 0
    assert t.append(MC.ITEM_A) == 0
    assert t.append(MC.ITEM_B) == 1
    assert t.root == MC.KNOWN1_ROOT
    assert t.proof(0).path == [MC.ITEM_B] and t.proof(1).path == [MC.ITEM_A]
    assert t.proof(0).address == [0] and t.proof(1).address == [1]
    assert t[0] == MC.ITEM_A and t[1] == MC.ITEM_B


def test_known_2pow28(M):
    t = M.MerkleTree(2 << 28)
    assert t.depth == 29
    t.append(MC.ITEM_A)
    assert t.root == MC.KNOWN29_ROOT_ONE
    t.append(MC.ITEM_B)
    assert t.root == MC.KNOWN29_ROOT_TWO
    assert t.proof(0).verify(t.root) and t.proof(1).verify(t.root)
    for (d, o), v in MC.KNOWN29_NODES.items():
        assert t.leaf(d, o) == v, (d, o)


def test_uniques(M):
    t = M.MerkleTree(2 << 28)
    for (d, o), v in MC.UNIQUES.items():
        assert t.leaf(d, o) == v == G.merkle_unique(d, o)


# ---------------------------------------------------------------- 4: incremental = bulk = Python
COUNTS = [1, 2, 3, 5, 8, 37, 256, 257, 1000]


@pytest.mark.parametrize("depth", [10, 29])
def test_bulk_build_equals_python_tree(M, depth):
    leaves = MC.random_leaves(max(COUNTS), 100 + depth)
    for n in COUNTS:
        ref = MC.PyTree(depth, leaves[:n])
        t = M.MerkleTree(1 << depth)
        t.extend(leaves[:n])                                       # n = 1000: level 1 has 500 parents -> the per-level kernel, then the tail
        MC.assert_same_nodes(t, ref)
        t.close()


@pytest.mark.parametrize("depth", [10, 29])
def test_chunked_appends_equal_bulk(M, depth):
    leaves = MC.random_leaves(1000, 200 + depth)
    for n, cuts in [(5, [1, 4]), (37, [16, 17]), (257, [1, 256]), (257, [255, 256]), (1000, [3, 640]), (1000, [513, 514])]:
        ref = MC.PyTree(depth, leaves[:n])
        t = M.MerkleTree(1 << depth)
        lo = 0
        for hi in cuts + [n]:
            t.extend(leaves[lo:hi])
            lo = hi
            if hi <= 40:
                assert t.root == MC.PyTree(depth, leaves[:hi]).root
        MC.assert_same_nodes(t, ref)
        t.close()
    ref = MC.PyTree(depth, leaves[:9])
    t = M.MerkleTree(1 << depth)
    for i, v in enumerate(leaves[:9]):                             # one by one
        assert t.append(v) == i
    MC.assert_same_nodes(t, ref)


def test_large_chunks_go_through_the_level_kernel(M, zk):
    """3 000 leaves at depth 12 in chunks 1 | 1 700 | 1 299: the second and third appends have several levels wider than a workgroup"""
    leaves = MC.random_leaves(3000, 31)
    with MC.make_pool() as pool:
        ref = MC.PyTree(12, leaves, pool)
    t = M.MerkleTree(1 << 12, reserve=16)                          # a small reservation: every level grows on the way
    t.extend(leaves[:1]); t.extend(leaves[1:1701]); t.extend(leaves[1701:])
    MC.assert_same_nodes(t, ref)
    # the same leaves from a device buffer, Montgomery and canonical
    for canonical in (False, True):
        buf = zk.DeviceBuffer(32 * 3000)
        buf.upload(F.ints_to_limbs(leaves) if canonical else F.fr_to_mont(leaves))
        t2 = M.MerkleTree(1 << 12)
        t2.extend(buf, canonical=canonical)
        assert t2.root == ref.root and len(t2) == 3000
        assert t2.leaf(0, 2999) == leaves[2999] and t2.leaf(5, 93) == ref.levels[5][93]
        t2.close(); buf.free()


def test_every_level_on_its_own_launch_gives_the_same_tree(M, monkeypatch):
    """ZK_MTREE_NO_TAIL=1 (the form the tail kernel is measured against) computes the same nodes"""
    leaves = MC.random_leaves(300, 8)
    ref = MC.PyTree(29, leaves)
    monkeypatch.setenv("ZK_MTREE_NO_TAIL", "1")
    t = M.MerkleTree(1 << 29)
    monkeypatch.delenv("ZK_MTREE_NO_TAIL")
    t.extend(leaves[:299]); t.append(leaves[299])
    MC.assert_same_nodes(t, ref)
    t.update_many([0, 299], [5, 6]); ref.set(0, 5); ref.set(299, 6)
    MC.assert_same_nodes(t, ref)


# ---------------------------------------------------------------- 5: updates
@pytest.mark.parametrize("depth", [10, 29])
def test_updates(M, depth):
    n = 37
    leaves = MC.random_leaves(n, 300 + depth)
    new = MC.random_leaves(64, 400 + depth)
    ref = MC.PyTree(depth, leaves)
    t = M.MerkleTree(1 << depth)
    t.extend(leaves)
    t.update(5, new[0]); ref.set(5, new[0])                        # single
    MC.assert_same_nodes(t, ref)
    t[36] = new[1]; ref.set(36, new[1])                            # the last leaf of an odd-sized level: its sibling is a placeholder
    MC.assert_same_nodes(t, ref)
    idx = [0, 1, 2, 3, 16, 17, 35, 36]                             # shared ancestors
    t.update_many(idx, new[2:10])
    for i, v in zip(idx, new[2:10]):
        ref.set(i, v)
    MC.assert_same_nodes(t, ref)
    t.update_many([7, 8, 7, 30, 7], new[10:15])                    # duplicates: the last write wins
    ref.set(8, new[11]); ref.set(30, new[13]); ref.set(7, new[14])
    MC.assert_same_nodes(t, ref)
    assert t[7] == new[14]


def test_update_wider_than_a_workgroup(M):
    """600 updated leaves of 1 000: the lower levels of the update go through k_mimc_merkle_update, the rest through the tail"""
    leaves = MC.random_leaves(1000, 51)
    new = MC.random_leaves(600, 52)
    idx = [(i * 617) % 1000 for i in range(600)]                  # distinct (617 is coprime to 1000), unsorted
    t = M.MerkleTree(1 << 29)
    t.extend(leaves)
    t.update_many(idx, new)
    for i, v in zip(idx, new):
        leaves[i] = v
    MC.assert_same_nodes(t, MC.PyTree(29, leaves))


# ---------------------------------------------------------------- 6: paths
@pytest.mark.parametrize("depth", [10, 29])
def test_paths(M, depth):
    leaves = MC.random_leaves(1000, 500 + depth)
    for n, sample in [(37, range(37)), (1000, [0, 1, 2, 255, 256, 511, 512, 640, 998, 999])]:
        ref = MC.PyTree(depth, leaves[:n])
        t = M.MerkleTree(1 << depth)
        t.extend(leaves[:n])
        ivs = G.merkle_ivs(29)
        for i, p in zip(sample, t.proofs(list(sample))):
            assert p.leaf == leaves[i] and p.address == ref.bits(i) and p.path == ref.path(i), i
            assert G.merkle_root(p.leaf, p.address, p.path, ivs) == ref.root
            assert p.verify(t.root)
        last = t.proof(n - 1)
        holes = ref.placeholder_levels(n - 1)
        assert holes and all(last.path[d] == G.merkle_unique(d, ((n - 1) >> d) ^ 1) for d in holes)
        assert t.proof(3) == t.proofs([3])[0]


# ---------------------------------------------------------------- 7: the hand-over to the witness planner
def test_fill_witnesses_then_witness_plan(zk, M):
    D, n, k = 29, 37, 3
    leaves = MC.random_leaves(n, 61)
    ref = MC.PyTree(D, leaves)
    t = M.MerkleTree(1 << D)
    t.extend(leaves)
    indices = [0, 36, 17]                                          # 36: the path holds placeholders
    cases = [G.merkle_membership_circuit(D, leaf=leaves[i], address=i, path=ref.path(i)) for i in indices]
    r = cases[0][0]
    assert all(c[2] == ref.root for c in cases)
    supplied = list(range(0, 1 + 1 + D + D + 1 + 29))              # ONE, root, address bits, path, leaf, IVs (allocation order)
    sentinel = np.arange(4 * (r.V + 1) * (k + 1), dtype=np.uint64).reshape(k + 1, r.V + 1, 4) + np.uint64(7)
    buf = zk.DeviceBuffer(32 * (r.V + 1) * (k + 1))
    buf.upload(sentinel)
    t.fill_witnesses(indices, buf, r)
    got = buf.download((k + 1, r.V + 1, 4))
    for p in range(k):
        assert np.array_equal(got[p, supplied], F.fr_to_mont([cases[p][1][v] for v in supplied])), p
        assert np.array_equal(got[p, len(supplied):], sentinel[p, len(supplied):])      # nothing else of the row was written
    assert np.array_equal(got[k], sentinel[k])
    plan = zk.WitnessPlan(r, supplied)
    assert plan.solve(buf.ptr, k) == 0
    got = buf.download((k + 1, r.V + 1, 4))
    for p in range(k):
        assert np.array_equal(got[p], F.fr_to_mont(cases[p][1])), p                  # element for element
    assert np.array_equal(got[k], sentinel[k])                                      # the row behind the batch is the caller's still
    # an explicit layout that puts the inputs elsewhere in a wider row
    L = M.Layout(70, 1, 31, 69, 80, 5)
    wide = np.zeros((2, 100, 4), dtype=np.uint64)
    buf2 = zk.DeviceBuffer(wide.nbytes)
    buf2.upload(wide)
    t.fill_witnesses([36, 1], buf2, L, row_elems=100)
    w = buf2.download((2, 100, 4))
    for p, i in enumerate([36, 1]):
        vals = F.fr_from_mont(w[p])
        assert vals[0] == 1 and vals[70] == ref.root and vals[69] == leaves[i]
        assert vals[1:1 + D] == ref.bits(i) and vals[31:31 + D] == ref.path(i) and vals[80:85] == G.merkle_ivs(29)[:5]
        assert vals[85:] == [0] * 15 and vals[60:69] == [0] * 9
    plan.close(); buf.free(); buf2.free()


# ---------------------------------------------------------------- 8: errors
def test_errors_leave_the_tree_as_it_was(zk, M):
    def code(fn, *a, **kw):
        with pytest.raises(zk.ZkError) as e:
            fn(*a, **kw)
        return e.value.code
    for n_items in (0, 1, 3, 6, 1 << 30):                          # depth 0, not a power of two, depth 30
        with pytest.raises((ValueError, zk.ZkError)):
            M.MerkleTree(n_items)
    h = C.c_void_p()
    for depth in (0, 30):
        assert zk._lib.zk_mtree_create(C.c_uint32(depth), C.c_uint64(0), 0, C.byref(h)) == 1 and not h.value
    leaves = MC.random_leaves(8, 71)
    ref = MC.PyTree(3, leaves[:5])
    t = M.MerkleTree(8)
    out = np.zeros(4, dtype=np.uint64)
    assert zk._lib.zk_mtree_root(t._h, zk._p64(out)) == 1          # the root of an empty tree is an error, not a value
    assert t.root is None
    t.extend(leaves[:5])
    assert code(t.extend, leaves[:4]) == 1                         # past the capacity: nothing is appended, not even the part that fits
    MC.assert_same_nodes(t, ref)
    assert code(t.update, 5, 1) == 1 and code(t.update_many, [0, 8], [1, 2]) == 1      # index >= size
    assert code(t.proofs, [5]) == 1 and code(t.proof, 1 << 40) == 1
    with pytest.raises(IndexError):
        t[5]
    bad = F.ints_to_limbs([1, F.FR])                               # leaf = r, as limbs (the int form is refused by the binding: ValueError)
    assert code(t.extend, bad) == 1 and code(t.update_many, [0, 1], bad) == 1
    with pytest.raises(ValueError):
        t.append(F.FR)
    with pytest.raises(ValueError):
        t.append(-1)
    dbuf = zk.DeviceBuffer(64)
    for canonical in (True, False):                                # resident leaves: the kernel counts them
        dbuf.upload(bad)
        assert code(t.extend, dbuf, canonical=canonical) == 1
    assert code(t.leaf, 4, 0) == 1 and code(t.leaf, 3, 1) == 1 and code(t.leaf, 0, 8) == 1
    wbuf = zk.DeviceBuffer(32 * 20)
    assert code(t.fill_witnesses, [0], wbuf.ptr, M.Layout(1, 2, 5, 8, 9, 29), row_elems=20) == 1       # IVs leave the row
    assert code(t.fill_witnesses, [0], wbuf.ptr, M.Layout(20, 2, 5, 8, 9, 3), row_elems=20) == 1       # root_var = row_elems
    assert code(t.fill_witnesses, [0], wbuf.ptr, M.Layout(1, 18, 5, 8, 9, 3), row_elems=20) == 1       # address bits leave the row
    assert code(t.fill_witnesses, [0], wbuf.ptr, M.Layout(1, 2, 5, 8, 9, 30), row_elems=2000) == 1     # more IVs than there are
    assert code(t.fill_witnesses, [7], wbuf.ptr, M.Layout(1, 2, 5, 8, 9, 3), row_elems=20) == 1        # index >= size
    MC.assert_same_nodes(t, ref)                                   # ... and after all of it the tree is what it was
    t.extend(leaves[5:])                                           # full now
    assert code(t.append, 1) == 1
    MC.assert_same_nodes(t, MC.PyTree(3, leaves))
    # null handles
    L, z = zk._lib, C.c_uint64(0)
    assert L.zk_mtree_size(None, C.byref(z)) == 1 and L.zk_mtree_append(None, zk._p64(out), C.c_uint64(1), 1) == 1
    assert L.zk_mtree_append_resident(None, C.c_void_p(dbuf.ptr), C.c_uint64(1), 1) == 1
    assert L.zk_mtree_update(None, zk._p64(out), zk._p64(out), C.c_uint32(1), 1) == 1
    assert L.zk_mtree_root(None, zk._p64(out)) == 1 and L.zk_mtree_node(None, C.c_uint32(0), C.c_uint64(0), zk._p64(out)) == 1
    assert L.zk_mtree_paths(None, zk._p64(out), C.c_uint32(1), zk._p64(out), zk._p64(out)) == 1
    lay = M.Layout(1, 2, 5, 8, 9, 3)
    assert L.zk_mtree_fill_witnesses(None, zk._p64(out), C.c_uint32(1), C.c_void_p(wbuf.ptr), C.c_uint64(20), C.byref(lay)) == 1
    assert L.zk_mtree_fill_witnesses(t._h, zk._p64(out), C.c_uint32(1), None, C.c_uint64(20), C.byref(lay)) == 1
    L.zk_mtree_free(None)
    dbuf.free(); wbuf.free()


def test_a_library_without_the_tree_is_a_clear_error(emul, zk):
    """the emulation build of the prover alone has no zk_mtree_*: the module says so instead of failing deep inside ctypes"""
    from ethsnarks_amd import merkle
    loaded = zk._lib_path_loaded
    zk._lib = None; zk._lib_path_loaded = None
    zk.load_library(emul)
    try:
        with pytest.raises(ImportError, match="no Merkle tree entry points"):
            merkle.MerkleTree(4)
    finally:
        zk._lib = None; zk._lib_path_loaded = None
        zk.load_library(loaded)
