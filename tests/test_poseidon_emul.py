"""Poseidon on the CPU emulation build of the HIP sources (csrc/poseidon.hpp, merkle.hpp, merkle.cpp; Field::ldot6 of bn254.hpp through the
arithmetic probe): constants, hashing, the width-2/3/4 tree and the hand-over to the witness planner and the prover, against the restatement of
the reference's permutation and tree in poseidon_cases.py.  Everything is integer arithmetic and compares exactly.  test_poseidon_gpu.py runs
the same checks on the device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F
import arith_ref as A
import merkle_cases as MC
import poseidon_cases as PC
import poseidon_checks as chk
from poseidon_checks import LDOT6



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


def code(zk, fn, *a, **kw):
    with pytest.raises(zk.ZkError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------- constants
def test_constants(M):
    chk.check_constants(M)


def test_the_reduction_is_exercised_and_stays_out_of_the_chain(M):
    """49 of the first 65 digests are >= r: the library's constants are the reduced digests of the UNREDUCED chain"""
    import hashlib
    lib_c, _ = M.poseidon_constants()
    s, above = b"poseidon_constants", 0
    for i in range(65):
        s = hashlib.blake2b(s, digest_size=32).digest()
        above += int.from_bytes(s, "little") >= F.FR
        assert int.from_bytes(s, "little") % F.FR == lib_c[i], i
    assert above == 49


# ---------------------------------------------------------------- hashing
def test_hashing(M):
    chk.check_hashing(M, 8)                                            # 5 x 8 = 40 random rows


def test_permute_twice(M):
    chk.check_permute(M, 5)


def test_hashing_errors(zk, M):
    top = (1 << 256) - 1
    for bad in (F.FR, top):
        for n_in, pos in [(1, 0), (2, 1), (5, 4)]:
            rows = F.ints_to_limbs([1] * (2 * n_in))
            rows[n_in + pos] = F.ints_to_limbs([bad])[0]           # in the second hash
            out = np.full((2, 4), 7, dtype=np.uint64)
            assert zk._lib.zk_poseidon_hash(zk._p64(rows), C.c_uint32(n_in), C.c_uint32(2), 0, zk._p64(out)) == 1
            assert (out == 7).all()
        st = F.ints_to_limbs([1] * 5 + [bad])
        keep = st.copy()
        assert zk._lib.zk_poseidon_permute(zk._p64(st), C.c_uint32(1), 0) == 1 and np.array_equal(st, keep)
    for n_in in (0, 6):
        rows = F.ints_to_limbs([1] * 6)
        out = np.full((1, 4), 7, dtype=np.uint64)
        assert zk._lib.zk_poseidon_hash(zk._p64(rows), C.c_uint32(n_in), C.c_uint32(1), 0, zk._p64(out)) == 1 and (out == 7).all()
    assert code(zk, M.poseidon_hash, [[1, 2, 3, 4, 5, 6]]) == 1
    assert zk._lib.zk_poseidon_hash(None, C.c_uint32(1), C.c_uint32(1), 0, None) == 1
    assert zk._lib.zk_poseidon_permute(None, C.c_uint32(1), 0) == 1
    assert zk._lib.zk_poseidon_constants(None, None) == 0


# ---------------------------------------------------------------- ldot6
@pytest.mark.parametrize("field", ["fr", "fq"])
def test_ldot6(zk, field):
    chk.check_ldot6(zk, field, loose=False)
    # the emulation's strict products take loose operands as well: the largest sum the precondition admits, as the device meets it
    p = A.MOD[field]
    op = (zk.PROBE_FR if field == "fr" else zk.PROBE_FQ) + LDOT6
    t = (2 * p - 1,) * 6 + (p - 1,) * 6
    g = F.limbs_to_ints(zk.arith_probe(op, F.ints_to_limbs(list(t)).reshape(1, 12, 4)).reshape(1, 4))[0]
    assert g < 2 * p and g % p == 6 * (2 * p - 1) * (p - 1) * pow(1 << 256, p - 2, p) % p


# ---------------------------------------------------------------- the tree
SHAPES = [(2, 5, [1, 2, 5, 31, 32]), (3, 3, [1, 2, 4, 10, 26, 27]), (4, 3, [1, 3, 5, 17, 63, 64])]


def new_tree(M, width, depth, **kw):
    return M.MerkleTree(width ** depth, width=width, hasher="poseidon", **kw)


@pytest.mark.parametrize("width,depth,counts", SHAPES, ids=["w2", "w3", "w4"])
def test_tree_bulk_and_chunked(zk, M, width, depth, counts):
    leaves = MC.random_leaves(max(counts), 900 + width)
    for n in counts:
        ref = PC.PyTree(depth, width, leaves[:n])
        t = new_tree(M, width, depth)
        assert t.root is None and (t.depth, t.width) == (depth, width)
        t.extend(leaves[:n])
        PC.assert_same_nodes(t, ref)
        t.close()
        cuts = sorted(set(c for c in (1, width, width + 1, n - 1, n // 2) if 0 < c < n))     # awkward: inside and at the edge of a node
        t = new_tree(M, width, depth, reserve=1)
        lo = 0
        for hi in cuts + [n]:
            t.extend(leaves[lo:hi])
            lo = hi
        PC.assert_same_nodes(t, ref)
        if n == width ** depth:                                    # a full tree refuses an append
            assert code(zk, t.append, 1) == 1
            PC.assert_same_nodes(t, ref)
        t.close()


@pytest.mark.parametrize("width,depth,counts", SHAPES, ids=["w2", "w3", "w4"])
def test_tree_updates(M, width, depth, counts):
    n = counts[-2]                                                 # one short of full: placeholders at the end of every level
    leaves = MC.random_leaves(n, 910 + width)
    new = MC.random_leaves(16, 920 + width)
    ref = PC.PyTree(depth, width, leaves)
    t = new_tree(M, width, depth)
    t.extend(leaves)
    t.update(n - 1, new[0]); ref.set(n - 1, new[0])                # the last leaf: its node ends in placeholders
    PC.assert_same_nodes(t, ref)
    idx = [0, 1, width - 1, width, n - 2, n - 1]                   # shared ancestors
    t.update_many(idx, new[1:7])
    for i, v in zip(idx, new[1:7]):
        ref.set(i, v)
    PC.assert_same_nodes(t, ref)
    t.update_many([3, 4, 3, n - 1, 3], new[7:12])                  # duplicates: the last write wins
    ref.set(4, new[8]); ref.set(n - 1, new[10]); ref.set(3, new[11])
    PC.assert_same_nodes(t, ref)
    assert t[3] == new[11]
    t.close()


@pytest.mark.parametrize("width,depth,counts", SHAPES, ids=["w2", "w3", "w4"])
def test_tree_proofs(M, width, depth, counts):
    for n in counts:
        leaves = MC.random_leaves(n, 930 + width)
        ref = PC.PyTree(depth, width, leaves)
        t = new_tree(M, width, depth)
        t.extend(leaves)
        proofs = t.proofs(range(n))
        for i, p in enumerate(proofs):
            assert p.leaf == leaves[i] and p.address == ref.digits(i) and p.path == ref.path(i) and p.width == width, (n, i)
            assert ref.verify(p.leaf, p.address, p.path) and p.verify(t.root)
        assert not proofs[0].verify((t.root + 1) % F.FR)
        holes = ref.placeholders(n - 1)
        if n < width ** depth:
            assert holes
        for d, offs in holes:
            sibs = proofs[-1].path[d] if width > 2 else [proofs[-1].path[d]]
            assert [G.merkle_unique(d, o) for o in offs] == sibs[len(sibs) - len(offs):]
        t.close()
    # more than one placeholder on a level at widths 3 and 4
    if width > 2:
        ref = PC.PyTree(depth, width, MC.random_leaves(1, 1))
        assert all(len(offs) == width - 1 for _, offs in ref.placeholders(0)) and len(ref.placeholders(0)) == depth


def test_creation_errors_and_info(zk, M):
    h = C.c_void_p()
    mk = lambda d, w, hs: zk._lib.zk_mtree_create_ex(C.c_uint32(d), C.c_uint32(w), hs, C.c_uint64(0), 0, C.byref(h))
    assert mk(3, 3, 0) == 1 and not h.value                       # MiMC at width 3
    assert mk(3, 5, 1) == 1 and mk(3, 1, 1) == 1 and not h.value   # Poseidon at width 5
    assert mk(15, 4, 1) == 1 and mk(19, 3, 1) == 1 and mk(30, 2, 1) == 1 and mk(0, 2, 1) == 1 and not h.value
    assert mk(3, 2, 2) == 1 and not h.value                       # no such hasher
    for w, d in [(2, 29), (3, 18), (4, 14)]:
        t = new_tree(M, w, d)
        dd, ww, hh = C.c_uint32(0), C.c_uint32(0), C.c_int(-1)
        assert zk._lib.zk_mtree_info(t._h, C.byref(dd), C.byref(ww), C.byref(hh)) == 0 and (dd.value, ww.value, hh.value) == (d, w, 1)
        t.append(5)
        assert t.root == PC.PyTree(d, w, [5]).root
        t.close()
    assert zk._lib.zk_mtree_info(None, None, None, None) == 1
    with pytest.raises(ValueError):
        M.MerkleTree(10, width=3, hasher="poseidon")
    t = new_tree(M, 3, 3)
    t.extend([1, 2, 3, 4])
    buf = zk.DeviceBuffer(32 * 64)
    assert code(zk, t.fill_witnesses, [0], buf.ptr, M.Layout(1, 2, 5, 8, 0, 0), row_elems=64) == 1      # no membership circuit at width 3
    t2 = new_tree(M, 2, 3)
    t2.extend([1, 2, 3])
    assert code(zk, t2.fill_witnesses, [0], buf.ptr, M.Layout(1, 2, 5, 8, 9, 3), row_elems=64) == 1     # Poseidon has no IVs to write
    t2.fill_witnesses([0], buf.ptr, M.Layout(1, 2, 5, 8, 0, 0), row_elems=64)
    t2.close()
    assert code(zk, t.update, 4, 1) == 1 and code(zk, t.proofs, [4]) == 1 and code(zk, t.leaf, 0, 27) == 1 and code(zk, t.leaf, 4, 0) == 1
    PC.assert_same_nodes(t, PC.PyTree(3, 3, [1, 2, 3, 4]))
    buf.free()


def test_mimc_tree_through_create_ex_equals_create(zk, M):
    leaves = MC.random_leaves(37, 940)
    a = M.MerkleTree(1 << 6)
    h = C.c_void_p()
    assert zk._lib.zk_mtree_create_ex(C.c_uint32(6), C.c_uint32(2), 0, C.c_uint64(0), 0, C.byref(h)) == 0
    b = M.MerkleTree.__new__(M.MerkleTree)
    b._h, b.depth, b.width, b.hasher, b.n_items, b.device = h, 6, 2, "mimc", 64, 0
    a.extend(leaves); b.extend(leaves)
    ref = MC.PyTree(6, leaves)
    MC.assert_same_nodes(a, ref); MC.assert_same_nodes(b, ref)
    assert a.proofs(range(37)) == b.proofs(range(37))


# ---------------------------------------------------------------- membership: tree -> fill_witnesses -> WitnessPlan -> prover
def test_membership_chain_depth_3(zk, M, oracle):
    D, n = 3, 7
    leaves = MC.random_leaves(n, 950)
    ref = PC.PyTree(D, 2, leaves)
    t = new_tree(M, 2, D)
    t.extend(leaves)
    indices = [0, 6, 3]                                            # 6: placeholders on its path
    assert ref.placeholders(6)
    cases = [G.poseidon_membership_circuit(D, leaf=leaves[i], address=i, path=ref.path(i)) for i in indices]
    r = cases[0][0]
    assert r.nC == 322 * D + 1 and all(c[2] == ref.root for c in cases)
    k = len(indices)
    supplied = list(range(0, 1 + 1 + D + D + 1))                   # ONE, root, address bits, path, leaf
    sentinel = np.arange(4 * (r.V + 1) * (k + 1), dtype=np.uint64).reshape(k + 1, r.V + 1, 4) + np.uint64(7)
    buf = zk.DeviceBuffer(32 * (r.V + 1) * (k + 1))
    buf.upload(sentinel)
    t.fill_witnesses(indices, buf, r)
    got = buf.download((k + 1, r.V + 1, 4))
    for p in range(k):
        assert np.array_equal(got[p, supplied], F.fr_to_mont([cases[p][1][v] for v in supplied])), p
        assert np.array_equal(got[p, len(supplied):], sentinel[p, len(supplied):])      # no IVs, nothing else
    plan = zk.WitnessPlan(r, supplied)
    assert plan.solve(buf.ptr, k) == 0
    got = buf.download((k + 1, r.V + 1, 4))
    for p in range(k):
        assert np.array_equal(got[p], F.fr_to_mont(cases[p][1])), p
    assert np.array_equal(got[k], sentinel[k])
    pk, vk = zk.keygen(r, seed=33)
    ctx = zk.ProverContext(pk, r)
    text = zk.prove(ctx, got[1])
    assert text == oracle.prove(oracle.pk_from_parts(pk.parts()), r, F.fr_to_mont(cases[1][1]))[0]
    assert zk.stub_verify(vk.to_json(), text)
    ctx.close(); plan.close(); buf.free()
