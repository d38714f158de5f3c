"""Poseidon on an MI355X (libzkhip.so): the checks of test_poseidon_emul.py on the device -- the hand-written gfx950 form of Field::ldot6, the
kernels of csrc/poseidon.hpp in both MIX forms -- trees at full depth for every width against the Python tree of poseidon_cases.py, and the resident
chain leaves -> Poseidon tree -> witnesses -> proofs -> verdicts.  Times are printed, never asserted."""
import json
import time
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F
import merkle_cases as MC
import poseidon_cases as PC
import poseidon_checks as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip):
    from ethsnarks_amd import merkle
    return merkle


@pytest.fixture(scope="module")
def pool():
    with MC.make_pool() as p:
        yield p


def test_constants_and_pinned_values(M):
    chk.check_constants(M)
    for inputs, want in PC.PINNED:
        assert M.poseidon_hash([inputs]) == [want]


@pytest.mark.parametrize("mix", ["dot6", "lmul", None])
def test_hashing_and_permute(M, monkeypatch, mix):
    """both MIX forms of the kernels (ZK_POSEIDON_MIX picks one per call; None: the form the tree uses)"""
    if mix:
        monkeypatch.setenv("ZK_POSEIDON_MIX", mix)
    chk.check_hashing(M, 60)                                         # 5 x 60 = 300 random rows
    chk.check_permute(M, 300)


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_ldot6(hip, field):
    chk.check_ldot6(hip, field, loose=True, extra_random=300)


def new_tree(M, width, depth, **kw):
    return M.MerkleTree(width ** depth, width=width, hasher="poseidon", **kw)


# n = 2^12 + 1 at width 2: levels 1 .. 3 have more than 256 parents (the level kernel), the rest goes through the tail; the extra leaf puts a
# placeholder at the end of every level.  700 updated leaves: more distinct parents than a workgroup holds on the lower levels (the update kernel)
@pytest.mark.parametrize("width,depth,n", [(2, 29, (1 << 12) + 1), (3, 18, 1000), (4, 14, 4097)], ids=["w2", "w3", "w4"])
def test_tree_against_python(M, hip, pool, width, depth, n):
    leaves = MC.random_leaves(n, 1000 + width)
    ref = PC.PyTree(depth, width, leaves, pool)
    t = new_tree(M, width, depth)
    before = hip.launch_count()
    t0 = time.perf_counter()
    t.extend(leaves)
    print("width %d depth %d, %d leaves: build %.2f ms, %d launches" % (width, depth, n, 1e3 * (time.perf_counter() - t0), hip.launch_count() - before))
    PC.assert_same_nodes(t, ref)
    sample = sorted(set([0, 1, width - 1, width, n // 2, n - 2, n - 1] + [(i * 7919) % n for i in range(20)]))
    for i, p in zip(sample, t.proofs(sample)):
        assert p.leaf == leaves[i] and p.address == ref.digits(i) and p.path == ref.path(i), i
        assert ref.verify(p.leaf, p.address, p.path)
    assert len(ref.placeholders(n - 1)) >= depth - 12
    new = MC.random_leaves(700, 1010 + width)
    idx = [(i * 617) % n for i in range(700)]
    idx[10] = idx[3]                                               # a duplicate: the last write wins
    t.update_many(idx, new)
    updated = list(leaves)
    for i, v in zip(idx, new):
        updated[i] = v
    PC.assert_same_nodes(t, PC.PyTree(depth, width, updated, pool))
    # the same leaves in chunks split inside a node
    t2 = new_tree(M, width, depth, reserve=4)
    for lo, hi in [(0, 1), (1, width + 1), (width + 1, n - 1), (n - 1, n)]:
        t2.extend(leaves[lo:hi])
    assert t2.root == ref.root and len(t2) == n


# ---------------------------------------------------------------- the resident chain at depth 29, width 2
def with_input(text, value):
    d = json.loads(text)
    d["input"] = ["0x%x" % value]
    return json.dumps(d)


def test_resident_chain_from_leaves_to_verdicts(M, hip, oracle, pool):
    D, n, k = 29, 300, 8
    r = G.poseidon_membership_circuit(D)[0]
    assert r.nC == 9339
    pk, vk = hip.keygen(r, seed=31)
    pk_o = oracle.pk_from_parts(pk.parts())
    ctx = hip.ProverContext(pk, r, max_batch=k)
    plan = hip.WitnessPlan(r, list(range(0, 1 + 1 + D + D + 1)))
    verifier = hip.Verifier(vk, max_batch=16)
    leaves = MC.random_leaves(n, 1020)
    t = new_tree(M, 2, D)
    t.extend(leaves)
    root_before = t.root
    t.update(100, 424242); leaves[100] = 424242
    ref = PC.PyTree(D, 2, leaves, pool)
    assert t.root == ref.root != root_before
    indices = [0, n - 1, 100, 101, 256, 77, 255, 3]
    buf = hip.DeviceBuffer(32 * (r.V + 1) * k)
    buf.upload(np.zeros((k, r.V + 1, 4), dtype=np.uint64))
    t0 = time.perf_counter()
    t.fill_witnesses(indices, buf, r)
    assert plan.solve(buf.ptr, k) == 0
    ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
    parts, _ = ctx.collect_batch(k)
    print("%d resident membership proofs (9 339 constraints): %.1f ms" % (k, 1e3 * (time.perf_counter() - t0)))
    w = buf.download((k, r.V + 1, 4))
    texts = [hip.proof_to_json(ctx.prove_combine(parts[p]), w[p][1:2]) for p in range(k)]
    for p, i in enumerate(indices):
        _, w_host, root = G.poseidon_membership_circuit(D, leaf=leaves[i], address=i, path=ref.path(i))
        wm = F.fr_to_mont(w_host)
        assert root == ref.root and np.array_equal(w[p], wm), i
        assert texts[p] == oracle.prove(pk_o, r, wm)[0], i         # byte-identical
        assert int(json.loads(texts[p])["input"][0], 16) == ref.root
    swapped = with_input(texts[1], root_before)                    # the root from before the update
    assert verifier.verify(texts + [swapped]) == [True] * k + [False]
    assert hip.stub_verify(vk.to_json(), texts[0]) and not hip.stub_verify(vk.to_json(), swapped)
    ctx.close(); plan.close(); verifier.close(); buf.free()


def test_cpp_wrapper_on_the_device(hip, tmp_path):
    import os
    from conftest import ROOT
    from test_poseidon_cpp import compile_cpp, run_trees
    lib = os.path.join(ROOT, "ethsnarks_amd")
    run_trees(compile_cpp(tmp_path, lib, ["zkhip"], [lib]))
