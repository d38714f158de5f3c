"""The device MiMC Merkle tree on an MI355X (libzkhip.so): the checks of test_merkle_emul.py at sizes the emulation cannot afford, a 2^20-leaf
tree against a root computed without the kernels, and the resident chain leaves -> tree -> paths -> witnesses -> proofs -> verdicts.
Yardsticks: the reference's known answers, gadgets.py and the Python tree of merkle_cases.py.  Times are printed, never asserted."""
import json
import os
import subprocess
import time
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F, r1cs as R
import merkle_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip):
    from ethsnarks_amd import merkle
    return merkle


@pytest.fixture(scope="module")
def pool():
    with MC.make_pool() as p:
        yield p


def test_mimc_hash2_against_gadgets(M):
    rng = R.SplitMix64(77)
    edge = [0, 1, F.FR - 1]
    trip = [(a, b, c) for a in edge for b in edge for c in edge] + [(rng.fr(), rng.fr(), rng.fr()) for _ in range(300)] + [(1, 1, 0)]
    got = M.mimc_hash2([t[0] for t in trip], [t[1] for t in trip], [t[2] for t in trip])
    assert got == [G.mimc_hash([a, b], c) for a, b, c in trip]
    assert got[-1] == 4087330248547221366577133490880315793780387749595119806283278576811074525767
    assert M.mimc_hash2([MC.ITEM_A], [MC.ITEM_B], [918403109389145570117360101535982733651217667914747213867238065296420114726]) == \
        [15683951496311901749339509118960676303290224812129752890706581988986633412003]
    rc, iv = M.mimc_constants()
    assert rc == G.mimc_constants() and iv == G.merkle_ivs(29)


def test_known_answers(M):
    t = M.MerkleTree(2)
    t.append(MC.ITEM_A); t.append(MC.ITEM_B)
    assert t.root == MC.KNOWN1_ROOT and t.proof(0).path == [MC.ITEM_B] and t.proof(1).path == [MC.ITEM_A]
    t = M.MerkleTree(2 << 28)
    assert t.root is None
    for (d, o), v in MC.UNIQUES.items():
        assert t.leaf(d, o) == v
    t.append(MC.ITEM_A)
    assert t.root == MC.KNOWN29_ROOT_ONE
    t.append(MC.ITEM_B)
    assert t.root == MC.KNOWN29_ROOT_TWO
    assert t.proof(0).verify(t.root) and t.proof(1).verify(t.root)
    for (d, o), v in MC.KNOWN29_NODES.items():
        assert t.leaf(d, o) == v, (d, o)


def test_tree_of_2p14_leaves_node_for_node(M, hip, pool):
    n = 1 << 14
    leaves = MC.random_leaves(n, 141)
    ref = MC.PyTree(29, leaves, pool)
    t = M.MerkleTree(1 << 29)
    before = hip.launch_count()
    t.extend(leaves)
    # ingest + the levels wider than a workgroup (2^13 .. 2^9 parents) + one tail launch for the other 24 levels
    assert hip.launch_count() - before == 1 + 5 + 1
    MC.assert_same_nodes(t, ref)
    # the same leaves in chunks at awkward split points, into a tree of depth 14 (full at the end)
    ref14 = MC.PyTree(14, leaves, pool)
    t14 = M.MerkleTree(n, reserve=8)
    for lo, hi in [(0, 1), (1, 2), (2, 5), (5, 4099), (4099, 4100), (4100, 16383), (16383, 16384)]:
        t14.extend(leaves[lo:hi])
    MC.assert_same_nodes(t14, ref14)
    with pytest.raises(hip.ZkError) as e:
        t14.append(1)
    assert e.value.code == 1
    # paths: sampled leaves, the last one included
    ivs = G.merkle_ivs(29)
    sample = [0, 1, 2, 4095, 4096, 8191, 12345, n - 2, n - 1]
    for i, p in zip(sample, t.proofs(sample)):
        assert p.leaf == leaves[i] and p.address == ref.bits(i) and p.path == ref.path(i)
        assert G.merkle_root(p.leaf, p.address, p.path, ivs) == ref.root
    assert ref.placeholder_levels(n - 1) == list(range(14, 29))
    # updates: single, shared ancestors, duplicates (last write wins), more distinct parents than a workgroup holds
    new = MC.random_leaves(700, 142)
    t.update(77, new[0]); ref.set(77, new[0])
    t.update_many([5, 4, 5, 16383, 5], new[1:6])
    ref.set(4, new[2]); ref.set(16383, new[4]); ref.set(5, new[5])
    idx = [(i * 7919) % n for i in range(690)]
    t.update_many(idx, new[6:696])
    for i, v in zip(idx, new[6:696]):
        ref.set(i, v)
    MC.assert_same_nodes(t, ref)


def test_odd_sized_trees(M):
    leaves = MC.random_leaves(1000, 143)
    for depth, n in [(10, 37), (29, 37), (10, 257), (29, 1000)]:
        ref = MC.PyTree(depth, leaves[:n])
        t = M.MerkleTree(1 << depth)
        t.extend(leaves[:n])
        MC.assert_same_nodes(t, ref)
        last = t.proof(n - 1)
        holes = ref.placeholder_levels(n - 1)
        assert holes and all(last.path[d] == G.merkle_unique(d, ((n - 1) >> d) ^ 1) for d in holes)
        assert all(p.verify(ref.root) for p in t.proofs(range(0, n, 7)))
        t[n - 1] = 99; ref.set(n - 1, 99)                          # the last leaf of an odd-sized level
        MC.assert_same_nodes(t, ref)


def test_tree_of_2p20_leaves(M, hip, pool):
    n = 1 << 20
    rng = R.SplitMix64(2020)
    limbs = np.zeros((n, 4), dtype=np.uint64)
    leaves = []
    for i in range(n):
        leaves.append(rng.fr())
    limbs = F.ints_to_limbs(leaves)
    t = M.MerkleTree(1 << 29, reserve=n)
    t0 = time.perf_counter()
    t.extend(limbs)
    build_s = time.perf_counter() - t0
    nodes = sum((n >> d) for d in range(1, 21)) + 9
    print("2^20 leaves at depth 29: build %.1f ms (%.2f G Fr products/s over %d nodes)" % (1e3 * build_s, nodes * 728 / build_s / 1e9, nodes))
    t0 = time.perf_counter()
    ref = MC.PyTree(29, leaves, pool)                              # the root without the kernels
    print("the Python tree over %d processes: %.1f s" % (min(MC.MAX_WORKERS, os.cpu_count() or 1), time.perf_counter() - t0))
    assert t.root == ref.root and len(t) == n
    sample = sorted(set([0, n - 1] + [rng.next() % n for _ in range(62)]))
    t0 = time.perf_counter()
    proofs = t.proofs(sample)
    paths_s = time.perf_counter() - t0
    ivs = G.merkle_ivs(29)
    for i, p in zip(sample, proofs):
        assert p.leaf == leaves[i] and G.merkle_root(p.leaf, p.address, p.path, ivs) == ref.root, i
    r = G.merkle_membership_circuit(29)[0]
    buf = hip.DeviceBuffer(32 * (r.V + 1) * len(sample))
    t0 = time.perf_counter()
    t.fill_witnesses(sample, buf, r)
    fill_s = time.perf_counter() - t0
    print("%d paths: %.2f ms (%.0f paths/s); fill_witnesses: %.2f ms" % (len(sample), 1e3 * paths_s, len(sample) / paths_s, 1e3 * fill_s))
    buf.free()


# ---------------------------------------------------------------- the resident chain
@pytest.fixture(scope="module")
def chain(hip, oracle):
    """the depth-29 membership circuit with a key, a prover context, the witness plan and a verifier (k <= 8)"""
    r = G.merkle_membership_circuit(29)[0]
    pk, vk = hip.keygen(r, seed=29)
    c = dict(r=r, pk_o=oracle.pk_from_parts(pk.parts()), vk=vk.to_json(), ctx=hip.ProverContext(pk, r, max_batch=8),
             plan=hip.WitnessPlan(r, list(range(0, 1 + 1 + 29 + 29 + 1 + 29))), verifier=hip.Verifier(vk, max_batch=16))
    yield c
    c["ctx"].close(); c["plan"].close(); c["verifier"].close()


def prove_resident(hip, c, tree, indices):
    """tree -> fill_witnesses -> WitnessPlan.solve -> submit_batch(device_ptr): the witnesses never visit the host; returns the proof texts
    (and the completed witnesses, downloaded for the comparison only)"""
    r, k = c["r"], len(indices)
    buf = hip.DeviceBuffer(32 * (r.V + 1) * k)
    buf.upload(np.zeros((k, r.V + 1, 4), dtype=np.uint64))
    tree.fill_witnesses(indices, buf, r)
    assert c["plan"].solve(buf.ptr, k) == 0
    c["ctx"].submit_batch(None, device_ptr=buf.ptr, k=k)
    parts, _ = c["ctx"].collect_batch(k)
    w = buf.download((k, r.V + 1, 4))
    buf.free()
    return [hip.proof_to_json(c["ctx"].prove_combine(parts[p]), w[p][1:2]) for p in range(k)], w


def with_input(text, value):
    d = json.loads(text)
    d["input"] = ["0x%x" % value]
    return json.dumps(d)


def test_resident_chain_from_leaves_to_verdicts(M, hip, oracle, chain, pool):
    n = 1 << 12
    leaves = MC.random_leaves(n, 151)
    t = M.MerkleTree(1 << 29)
    t.extend(leaves)
    root_before = t.root
    t.update(1000, 424242); leaves[1000] = 424242
    ref = MC.PyTree(29, leaves, pool)
    assert t.root == ref.root != root_before
    indices = [0, n - 1, 1000, 1001, 2048, 77, 4000, 3]            # n - 1 (like all of them): placeholders on the levels 12 .. 28
    assert ref.placeholder_levels(n - 1) == list(range(12, 29))
    texts, w = prove_resident(hip, chain, t, indices)
    for p, i in enumerate(indices):
        _, w_host, root = G.merkle_membership_circuit(29, leaf=leaves[i], address=i, path=ref.path(i))      # the host front end, the Python tree's path
        wm = F.fr_to_mont(w_host)
        assert root == ref.root and np.array_equal(w[p], wm), i
        assert texts[p] == oracle.prove(chain["pk_o"], chain["r"], wm)[0], i                                  # byte-identical
        assert int(json.loads(texts[p])["input"][0], 16) == ref.root
    swapped = with_input(texts[1], root_before)                    # the root of the tree before the update
    assert chain["verifier"].verify(texts + [swapped]) == [True] * len(indices) + [False]
    assert hip.stub_verify(chain["vk"], texts[0]) and not hip.stub_verify(chain["vk"], swapped)


def test_proofs_after_update_many(M, hip, chain):
    n = 300
    leaves = MC.random_leaves(n, 161)
    t = M.MerkleTree(1 << 29)
    t.extend(leaves)
    old_root = t.root
    old_texts, _ = prove_resident(hip, chain, t, [5, 299])
    assert chain["verifier"].verify(old_texts) == [True, True]
    touched = [5, 6, 150, 299]
    new = MC.random_leaves(4, 162)
    t.update_many(touched, new)
    for i, v in zip(touched, new):
        leaves[i] = v
    ref = MC.PyTree(29, leaves)
    assert t.root == ref.root != old_root
    texts, _ = prove_resident(hip, chain, t, [5, 299, 7, 200])      # touched and untouched leaves against the new root
    assert all(int(json.loads(x)["input"][0], 16) == ref.root for x in texts)
    stale = with_input(old_texts[0], ref.root)                     # an old proof presented with the new root
    assert chain["verifier"].verify(texts + [stale, old_texts[1]]) == [True] * 4 + [False, True]


def test_cpp_wrapper_on_the_device(hip, tmp_path):
    from conftest import ROOT
    from test_merkle_cpp import compile_cpp, cpp_args
    lib = os.path.join(ROOT, "ethsnarks_amd")
    exe = compile_cpp(tmp_path, lib, ["zkhip"], [lib])
    p = subprocess.run([exe] + cpp_args(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "MTREE OK", p.stdout + p.stderr
