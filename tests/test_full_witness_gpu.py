"""MerkleTree.fill_full_witnesses on an MI355X (libzkhip.so): the checks of test_full_witness_emul.py at depth 3 on the device, and at depth 29 the
shape at which the lane-to-(row, level) mapping of k_mtree_fill_levels can go wrong -- k = 5 rows x 29 levels = 145 lanes: three workgroups of 64,
the last one partial, rows that straddle workgroups -- against the existing fill_witnesses + WitnessPlan.solve path, byte for byte."""
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import merkle_cases as MC
import full_witness_checks as chk
from full_witness_checks import HASHERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip):
    from ethsnarks_amd import merkle
    return merkle


# ---------------------------------------------------------------- depth 3: cases 1 - 3 of the emulation tests
@pytest.fixture(scope="module")
def depth3(hip, M):
    out = {h: chk.check_rows_against_gadgets(hip, M, h, 3, 7, [0, 6, 3], 960) for h in HASHERS}
    yield out
    for t, _, _, _ in out.values():
        t.close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_rows_equal_the_gadgets_witness(hip, M, depth3, hasher):
    assert hasher in depth3                                        # n = 7, indices [0, 6, 3]: checked by the fixture
    chk.check_rows_against_gadgets(hip, M, hasher, 3, 8, [7], 961)[0].close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_same_bytes_as_fill_witnesses_and_solve(hip, depth3, hasher):
    t, r, _, got = depth3[hasher]
    assert np.array_equal(chk.solved(hip, t, [0, 6, 3], r, hasher), got)


@pytest.mark.parametrize("hasher", HASHERS)
def test_one_row_proves(hip, oracle, depth3, hasher):
    _, r, cases, got = depth3[hasher]
    chk.check_proof(hip, oracle, r, cases[1][1], got[1])


# ---------------------------------------------------------------- depth 29
D, N, INDICES = 29, 70, [0, 1, 37, 64, 69]


@pytest.fixture(scope="module")
def depth29(hip, M):
    """per hasher: the tree of 70 leaves, the depth-29 circuit (built once, over leaf 0, so its witness is row 0's), the rows of both paths"""
    out = {}
    leaves = MC.random_leaves(N, 970)
    with MC.make_pool() as pool:
        for hasher in HASHERS:
            ref = chk.ref_tree(hasher, D, leaves, pool)
            t = chk.new_tree(M, hasher, D, leaves)
            r, w0, root = chk.circuit(hasher, D, leaves[0], 0, ref.path(0))
            assert root == ref.root == t.root and r.V + 1 == M.membership_full_layout(D, hasher)[3]
            out[hasher] = (t, r, w0, chk.filled(hip, t, INDICES, r), chk.solved(hip, t, INDICES, r, hasher))
    yield out
    for v in out.values():
        v[0].close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_depth_29_rows_straddling_workgroups(depth29, hasher):
    _, r, w0, (s, got), want = depth29[hasher]
    k = len(INDICES)
    assert k * D == 145
    for p in range(k):
        assert np.array_equal(got[p], want[p]), (hasher, INDICES[p])
    assert np.array_equal(got[k], s[k]) and np.array_equal(want[k], s[k])
    assert np.array_equal(got[0], F.fr_to_mont(w0))


def test_depth_29_poseidon_proofs_from_both_buffers(hip, depth29):
    """tree -> fill_full_witnesses -> submit_batch(device_ptr=...) gives the proofs of tree -> fill_witnesses -> solve -> submit_batch"""
    t, r, _, _, _ = depth29["poseidon"]
    k = len(INDICES)
    pk, _ = hip.keygen(r, seed=31)
    ctx = hip.ProverContext(pk, r, max_batch=k)
    plan = hip.WitnessPlan(r, list(range(chk.n_supplied("poseidon", D))))
    texts = []
    for full in (True, False):
        buf = hip.DeviceBuffer(32 * (r.V + 1) * k)
        buf.upload(np.zeros((k, r.V + 1, 4), dtype=np.uint64))
        if full:
            t.fill_full_witnesses(INDICES, buf, r)
        else:
            t.fill_witnesses(INDICES, buf, r)
            assert plan.solve(buf.ptr, k) == 0
        ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
        parts, _ = ctx.collect_batch(k)
        w = buf.download((k, r.V + 1, 4))
        texts.append([hip.proof_to_json(ctx.prove_combine(parts[p]), w[p][1:2]) for p in range(k)])
        buf.free()
    assert texts[0] == texts[1] and len(set(texts[0])) == k
    ctx.close(); plan.close()


def test_cpp_wrapper_on_the_device(hip, tmp_path):
    import os
    from conftest import ROOT
    from test_full_witness_cpp import compile_cpp, run_hasher
    lib = os.path.join(ROOT, "ethsnarks_amd")
    exe = compile_cpp(tmp_path, lib, ["zkhip"], [lib])
    for hasher in HASHERS:
        run_hasher(exe, hasher)
