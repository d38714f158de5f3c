"""What test_full_witness_emul.py and test_full_witness_gpu.py share: MerkleTree.fill_full_witnesses against the witness of the Python gadgets
(gadgets.merkle_membership_circuit / poseidon_membership_circuit) and against fill_witnesses + WitnessPlan.solve, byte for byte."""
import numpy as np
from ethsnarks_amd import gadgets as G, fields as F
import merkle_cases as MC
import poseidon_cases as PC

HASHERS = ("mimc", "poseidon")
STRIDE = {"mimc": 736, "poseidon": 322}


def n_supplied(hasher, D):
    """ONE, root, address bits, path, leaf (and the 29 IVs of the MiMC circuit): what fill_witnesses writes and WitnessPlan takes as known"""
    return 3 + 2 * D + (29 if hasher == "mimc" else 0)


def ref_tree(hasher, D, leaves, pool=None):
    return MC.PyTree(D, leaves, pool) if hasher == "mimc" else PC.PyTree(D, 2, leaves, pool)


def new_tree(M, hasher, D, leaves):
    t = M.MerkleTree(1 << D, hasher=hasher)
    t.extend(leaves)
    return t


def circuit(hasher, D, leaf, address, path):
    """(r1cs, witness, root) of the membership circuit of one leaf"""
    f = G.merkle_membership_circuit if hasher == "mimc" else G.poseidon_membership_circuit
    return f(D, leaf=leaf, address=address, path=path)


def sentinel(rows, elems):
    return np.arange(4 * elems * rows, dtype=np.uint64).reshape(rows, elems, 4) + np.uint64(7)


def filled(zk, t, indices, r=None, row_elems=None, **kw):
    """(sentinel, buffer after fill_full_witnesses) of k + 1 rows"""
    elems = row_elems if row_elems is not None else r.V + 1
    k = len(indices)
    s = sentinel(k + 1, elems)
    buf = zk.DeviceBuffer(32 * elems * (k + 1))
    buf.upload(s)
    t.fill_full_witnesses(indices, buf, r, row_elems=row_elems, **kw)
    got = buf.download((k + 1, elems, 4))
    buf.free()
    return s, got


def solved(zk, t, indices, r, hasher):
    """the same rows by the existing path: fill_witnesses, then WitnessPlan.solve over the same sentinel"""
    k = len(indices)
    s = sentinel(k + 1, r.V + 1)
    buf = zk.DeviceBuffer(32 * (r.V + 1) * (k + 1))
    buf.upload(s)
    t.fill_witnesses(indices, buf, r)
    plan = zk.WitnessPlan(r, list(range(n_supplied(hasher, t.depth))))
    assert plan.solve(buf.ptr, k) == 0
    got = buf.download((k + 1, r.V + 1, 4))
    plan.close(); buf.free()
    return got


def check_rows_against_gadgets(zk, M, hasher, D, n, indices, seed):
    """case 1: every row equals fr_to_mont of the front end's witness over all V + 1 elements; row k and the tail of a longer row keep the
    sentinel.  Returns (r1cs, the witnesses, the filled rows) for the checks that follow"""
    leaves = MC.random_leaves(n, seed)
    ref = ref_tree(hasher, D, leaves)
    t = new_tree(M, hasher, D, leaves)
    cases = [circuit(hasher, D, leaves[i], i, ref.path(i)) for i in indices]
    r, k = cases[0][0], len(indices)
    layout, var0, stride, elems = M.membership_full_layout(D, hasher)
    assert (var0, stride, elems) == (n_supplied(hasher, D), STRIDE[hasher], r.V + 1) and all(c[2] == ref.root == t.root for c in cases)
    s, got = filled(zk, t, indices, r)
    for p in range(k):
        assert np.array_equal(got[p], F.fr_to_mont(cases[p][1])), (hasher, n, indices[p])
    assert np.array_equal(got[k], s[k])
    tail = 5
    s2, got2 = filled(zk, t, indices, r, row_elems=r.V + 1 + tail)
    assert np.array_equal(got2[:k, :r.V + 1], got[:k]) and np.array_equal(got2[:, r.V + 1:], s2[:, r.V + 1:]) and np.array_equal(got2[k], s2[k])
    return t, r, cases, got


def check_proof(zk, oracle, r, witness, row, seed=33):
    """case 3: the filled row proves, the proof text is the oracle's, and it verifies"""
    pk, vk = zk.keygen(r, seed=seed)
    ctx = zk.ProverContext(pk, r)
    text = zk.prove(ctx, row)
    assert text == oracle.prove(oracle.pk_from_parts(pk.parts()), r, F.fr_to_mont(witness))[0]
    assert zk.stub_verify(vk.to_json(), text)
    ctx.close()
