"""MerkleTree.update_seq (zk_mtree_update_seq; the k_mtree_useq_* kernels of csrc/merkle.hpp) and gadgets.merkle_update_circuit on the CPU
emulation build: ordered leaf updates whose every occurrence sees its predecessors, and per update the complete witness of the root-to-root
transition circuit.  References (merkle_update_cases.py): the PyTree updated one set() at a time, the Python gadgets' witness, and inputs +
WitnessPlan.solve.  Integer arithmetic throughout; every comparison is exact.  test_merkle_update_gpu.py runs the same checks on the device."""
import numpy as np
import pytest
from ethsnarks_amd import fields as F, gadgets as G
import merkle_cases as MC
import merkle_update_cases as UC
import merkle_update_checks as chk
from merkle_update_cases import HASHERS
from test_full_witness_emul import emul_merkle, zk, M, no_guard_violations  # noqa: F401  (fixtures)


# ---------------------------------------------------------------- 1: the circuit alone
@pytest.fixture(scope="module")
def circuits3():
    """per hasher the depth-3 update circuit of leaf 5 of a 7-leaf tree: (r1cs, witness, roots, the PyTree before)"""
    out = {}
    leaves = MC.random_leaves(7, 1200)
    for hasher in HASHERS:
        ref = UC.ref_tree(hasher, 3, leaves)
        out[hasher] = G.merkle_update_circuit(3, hasher, old_leaf=leaves[5], new_leaf=12345, address=5, path=ref.path(5)) + (ref,)
    return out


@pytest.mark.parametrize("hasher", HASHERS)
def test_circuit_is_satisfied_and_laid_out_as_documented(circuits3, hasher):
    from ethsnarks_amd import merkle
    r, w, roots, ref = circuits3[hasher]
    D, per = 3, UC.STRIDE[hasher]
    assert r.is_satisfied(w) and r.nIn == 2 and r.nC == 2 * D * per + 2
    layout, var0, stride, elems = merkle.update_layout(D, hasher)
    assert (var0, stride, elems) == (UC.n_supplied(hasher, D), per, r.V + 1)
    assert roots[0] == ref.root and w[layout.old_root_var] == roots[0] and w[layout.new_root_var] == roots[1]
    assert w[layout.addr_var0:layout.addr_var0 + D] == [1, 0, 1] and w[layout.path_var0:layout.path_var0 + D] == ref.path(5)
    assert w[layout.old_leaf_var] == ref.node(0, 5) and w[layout.new_leaf_var] == 12345
    if hasher == "mimc":
        assert w[layout.iv_var0:layout.iv_var0 + layout.n_iv] == MC.IVS and layout.n_iv == 29
    ref.set(5, 12345)
    assert roots[1] == ref.root
    # the last variable of each chain is its result: the level blocks are where update_layout says
    if hasher == "poseidon":
        assert w[var0 + D * stride - 1] == roots[0] and w[var0 + 2 * D * stride - 1] == roots[1]
    else:
        assert w[var0 + (D - 1) * stride + 7] == roots[0] and w[var0 + (2 * D - 1) * stride + 7] == roots[1]     # selector 6, outputs[0], outputs[1]


@pytest.mark.parametrize("hasher", HASHERS)
def test_circuit_rejects_a_wrong_root_or_path(circuits3, hasher):
    r, w, _, _ = circuits3[hasher]
    for var in (2, 3 + 3 + 1):                                     # new_root; path[1]
        bad = list(w)
        bad[var] = (bad[var] + 1) % F.FR
        assert not r.is_satisfied(bad)


@pytest.mark.parametrize("hasher,depth", [("mimc", 29), ("poseidon", 29)])
def test_constraint_counts_at_depth_29(hasher, depth):
    r = G.merkle_update_circuit(depth, hasher)[0]
    assert r.nC == {"mimc": 42690, "poseidon": 18678}[hasher] == 2 * depth * UC.STRIDE[hasher] + 2


@pytest.mark.parametrize("hasher", HASHERS)
def test_planner_reproduces_the_witness_from_the_inputs(zk, circuits3, hasher):
    r, w, _, _ = circuits3[hasher]
    n_in = UC.n_supplied(hasher, 3)
    s = chk.sentinel(1, r.V + 1)
    s[0, :n_in] = F.fr_to_mont(w[:n_in])
    buf = zk.DeviceBuffer(s.nbytes)
    buf.upload(s)
    plan = zk.WitnessPlan(r, list(range(n_in)))
    assert plan.solve(buf.ptr, 1) == 0
    assert np.array_equal(buf.download(s.shape)[0], F.fr_to_mont(w))
    plan.close(); buf.free()


# ---------------------------------------------------------------- 2 - 4: the shapes of depth 3
@pytest.fixture(scope="module")
def shapes(zk, M):
    """per hasher: the case, its reference with the gadget witness of EVERY row, the constraint system, the tree and rows update_seq left"""
    case = UC.shapes_case()
    out = {}
    for hasher in HASHERS:
        ref = UC.reference(hasher, case, rows=range(len(case.indices)))
        assert ref.roots[4] == ref.roots[5] and len(set(ref.roots)) == len(ref.roots) - 1      # update 4 is the no-op
        r = ref.circuits[0][0]
        out[hasher] = (case, ref, r) + chk.check_case(zk, M, hasher, case, ref, r)
    yield out
    for v in out.values():
        v[3].close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_rows_roots_and_nodes_of_every_shape(zk, M, shapes, hasher):
    case, ref, r, _, _, got = shapes[hasher]                       # rows, roots, nodes: checked by the fixture
    chk.check_tail_untouched(zk, M, hasher, case, r, got)
    chk.check_single_updates_agree(M, hasher, case, ref)


@pytest.mark.parametrize("hasher", HASHERS)
def test_rows_are_what_the_planner_leaves(zk, shapes, hasher):
    case, ref, r, _, _, got = shapes[hasher]
    assert np.array_equal(chk.solved_rows(zk, r, hasher, case.depth, ref), got)


@pytest.mark.parametrize("hasher", HASHERS)
def test_one_row_proves(zk, oracle, shapes, hasher):
    _, ref, r, _, roots, got = shapes[hasher]
    assert ref.circuits[2][1][1:3] == roots[2:4]                   # row 2, the repeated index: public inputs (old_root, new_root)
    chk.check_proof(zk, oracle, r, ref.circuits[2][1], got[2])


# ---------------------------------------------------------------- 5, 6: one update; collisions on every level; above TAIL_BLOCK
@pytest.mark.parametrize("hasher", HASHERS)
def test_a_single_update(zk, M, shapes, hasher):
    case = UC.single_case()
    ref = UC.reference(hasher, case, rows=[0])
    chk.check_case(zk, M, hasher, case, ref, shapes[hasher][2])[0].close()


@pytest.fixture(scope="module")
def random70():
    """the case of 70 random updates of 16 leaves and, per hasher, its reference with the gadget witness of every row"""
    case = UC.random_case(4, 16, 70, 1220)
    assert all(len({a >> d for a in case.indices}) < 70 for d in range(5)) and len(set(case.indices)) == 16
    with MC.make_pool() as pool:
        return case, {h: UC.reference(h, case, rows=range(70), pool=pool) for h in HASHERS}


@pytest.mark.parametrize("no_tail", [False, True], ids=["tail", "launch_per_level"])
@pytest.mark.parametrize("hasher", HASHERS)
def test_70_random_updates_of_16_leaves(zk, M, random70, hasher, no_tail):
    """collisions on every level; launch_per_level: two workgroups of LEVEL_BLOCK per step of phase 1"""
    case, refs = random70
    chk.check_case(zk, M, hasher, case, refs[hasher], refs[hasher].circuits[0][0], no_tail=no_tail)[0].close()


def test_300_updates_launch_per_level(zk, M, shapes):
    """k above TAIL_BLOCK: phase 1 is one launch per level"""
    case = UC.random_case(3, 8, 300, 1230)
    ref = UC.reference("mimc", case, rows=(0, 150, 299))
    chk.check_case(zk, M, "mimc", case, ref, shapes["mimc"][2])[0].close()


# ---------------------------------------------------------------- 7: depth 29 (Poseidon here; both hashers on the device)
def test_depth_29_rows_straddling_workgroups(zk, M):
    hasher, case = "poseidon", UC.depth29_case()
    k = len(case.indices)
    assert k * case.depth * 2 == 290
    with MC.make_pool() as pool:
        ref = UC.reference(hasher, case, rows=[0], pool=pool)
    r = ref.circuits[0][0]
    t, _, got = chk.check_case(zk, M, hasher, case, ref, r)
    want = chk.solved_rows(zk, r, hasher, case.depth, ref)
    for j in range(k):
        assert np.array_equal(got[j], want[j]), j
    assert np.array_equal(got[k], want[k])
    t.close()


# ---------------------------------------------------------------- 9: refusals
@pytest.mark.parametrize("hasher", HASHERS)
def test_bad_arguments_are_refused_and_change_nothing(zk, M, hasher):
    chk.check_refusals(zk, M, hasher, UC.shapes_case())


def test_wide_poseidon_trees_are_refused(zk, M):
    chk.check_wide_tree_refused(zk, M)
