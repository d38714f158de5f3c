"""MerkleTree.update_seq on an MI355X (libzkhip.so): the checks of test_merkle_update_emul.py on the device for both hashers -- the shapes of depth 3,
one and 70 updates (one workgroup, and one launch per level with two workgroups), 300 updates (above TAIL_BLOCK), depth 29 where the
(row, level, side) lanes of the trace pass straddle workgroups -- and what only the device can show: the rows prove as a batch straight from
the buffer update_seq wrote."""
import os
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import merkle_cases as MC
import merkle_update_cases as UC
import merkle_update_checks as chk
from merkle_update_cases import HASHERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(hip):
    from ethsnarks_amd import merkle
    return merkle


# ---------------------------------------------------------------- 2 - 4: the shapes of depth 3
@pytest.fixture(scope="module")
def shapes(hip, M):
    case = UC.shapes_case()
    out = {}
    for hasher in HASHERS:
        ref = UC.reference(hasher, case, rows=range(len(case.indices)))
        assert ref.roots[4] == ref.roots[5] and len(set(ref.roots)) == len(ref.roots) - 1      # update 4 is the no-op
        r = ref.circuits[0][0]
        out[hasher] = (case, ref, r) + chk.check_case(hip, M, hasher, case, ref, r)
    yield out
    for v in out.values():
        v[3].close()


@pytest.mark.parametrize("hasher", HASHERS)
def test_rows_roots_and_nodes_of_every_shape(hip, M, shapes, hasher):
    case, ref, r, _, _, got = shapes[hasher]                       # rows, roots, nodes: checked by the fixture
    chk.check_tail_untouched(hip, M, hasher, case, r, got)
    chk.check_single_updates_agree(M, hasher, case, ref)


@pytest.mark.parametrize("hasher", HASHERS)
def test_rows_are_what_the_planner_leaves(hip, shapes, hasher):
    case, ref, r, _, _, got = shapes[hasher]
    assert np.array_equal(chk.solved_rows(hip, r, hasher, case.depth, ref), got)


@pytest.mark.parametrize("hasher", HASHERS)
def test_one_row_proves(hip, oracle, shapes, hasher):
    _, ref, r, _, roots, got = shapes[hasher]
    assert ref.circuits[2][1][1:3] == roots[2:4]                   # row 2, the repeated index: public inputs (old_root, new_root)
    chk.check_proof(hip, oracle, r, ref.circuits[2][1], got[2])


# ---------------------------------------------------------------- 5, 6
@pytest.mark.parametrize("hasher", HASHERS)
def test_a_single_update(hip, M, shapes, hasher):
    case = UC.single_case()
    ref = UC.reference(hasher, case, rows=[0])
    chk.check_case(hip, M, hasher, case, ref, shapes[hasher][2])[0].close()


@pytest.fixture(scope="module")
def random70():
    case = UC.random_case(4, 16, 70, 1220)
    assert all(len({a >> d for a in case.indices}) < 70 for d in range(5)) and len(set(case.indices)) == 16
    with MC.make_pool() as pool:
        return case, {h: UC.reference(h, case, rows=range(70), pool=pool) for h in HASHERS}


@pytest.mark.parametrize("no_tail", [False, True], ids=["tail", "launch_per_level"])
@pytest.mark.parametrize("hasher", HASHERS)
def test_70_random_updates_of_16_leaves(hip, M, random70, hasher, no_tail):
    """collisions on every level; launch_per_level: two workgroups of LEVEL_BLOCK per step of phase 1"""
    case, refs = random70
    chk.check_case(hip, M, hasher, case, refs[hasher], refs[hasher].circuits[0][0], no_tail=no_tail)[0].close()


def test_300_updates_launch_per_level(hip, M, shapes):
    """k above TAIL_BLOCK: phase 1 is one launch per level"""
    case = UC.random_case(3, 8, 300, 1230)
    ref = UC.reference("mimc", case, rows=(0, 150, 299))
    chk.check_case(hip, M, "mimc", case, ref, shapes["mimc"][2])[0].close()


# ---------------------------------------------------------------- 7, 8: depth 29
@pytest.fixture(scope="module")
def depth29(hip, M):
    """per hasher: the reference (row 0 with its gadget witness), the circuit, the rows of update_seq and of inputs + WitnessPlan.solve"""
    case = UC.depth29_case()
    assert len(case.indices) * case.depth * 2 == 290
    out = {}
    with MC.make_pool() as pool:
        refs = {h: UC.reference(h, case, rows=[0], pool=pool) for h in HASHERS}
    for hasher in HASHERS:
        ref = refs[hasher]
        r = ref.circuits[0][0]
        t, _, got = chk.check_case(hip, M, hasher, case, ref, r)
        t.close()
        out[hasher] = (case, ref, r, got, chk.solved_rows(hip, r, hasher, case.depth, ref))
    return out


@pytest.mark.parametrize("hasher", HASHERS)
def test_depth_29_rows_straddling_workgroups(depth29, hasher):
    case, ref, r, got, want = depth29[hasher]
    k = len(case.indices)
    for j in range(k):
        assert np.array_equal(got[j], want[j]), (hasher, j)
    assert np.array_equal(got[k], want[k])
    assert np.array_equal(got[0], F.fr_to_mont(ref.circuits[0][1]))


def test_depth_29_poseidon_batch_proofs_from_both_buffers(hip, M, depth29):
    """tree -> update_seq -> submit_batch(device_ptr=...) on the buffer update_seq wrote, with no host round trip in between, gives the proofs of
    inputs -> WitnessPlan.solve -> submit_batch: five distinct proofs that verify with public inputs (old_root, new_root)"""
    case, ref, r, _, _ = depth29["poseidon"]
    k, D = len(case.indices), case.depth
    n_in = UC.n_supplied("poseidon", D)
    pk, vk = hip.keygen(r, seed=31)
    ctx = hip.ProverContext(pk, r, max_batch=k)
    plan = hip.WitnessPlan(r, list(range(n_in)))
    texts = []
    for from_tree in (True, False):
        buf = hip.DeviceBuffer(32 * (r.V + 1) * k)
        rows = np.zeros((k, r.V + 1, 4), dtype=np.uint64)
        if from_tree:
            buf.upload(rows)
            t = chk.new_tree(M, "poseidon", case)
            assert t.update_seq(case.indices, case.values, buf, r) == ref.roots
            t.close()
        else:
            for j, row in enumerate(ref.inputs):
                rows[j, :n_in] = F.fr_to_mont(row)
            buf.upload(rows)
            assert plan.solve(buf.ptr, k) == 0
        ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
        parts, _ = ctx.collect_batch(k)
        w = buf.download((k, r.V + 1, 4))                          # the public inputs, read back from the buffer that was proved
        for j in range(k):
            assert np.array_equal(w[j, 1:3], F.fr_to_mont(ref.roots[j:j + 2]))
        texts.append([hip.proof_to_json(ctx.prove_combine(parts[p]), w[p][1:3]) for p in range(k)])
        buf.free()
    assert texts[0] == texts[1] and len(set(texts[0])) == k
    vkj = vk.to_json()
    assert all(hip.stub_verify(vkj, text) for text in texts[0])
    ctx.close(); plan.close()


# ---------------------------------------------------------------- 9: refusals
@pytest.mark.parametrize("hasher", HASHERS)
def test_bad_arguments_are_refused_and_change_nothing(hip, M, hasher):
    chk.check_refusals(hip, M, hasher, UC.shapes_case())


def test_wide_poseidon_trees_are_refused(hip, M):
    chk.check_wide_tree_refused(hip, M)


# ---------------------------------------------------------------- 10: the C++ wrapper
def test_cpp_wrapper_on_the_device(hip, M, tmp_path):
    from conftest import ROOT
    from test_merkle_update_cpp import compile_cpp, run_hasher
    lib = os.path.join(ROOT, "ethsnarks_amd")
    exe = compile_cpp(tmp_path, lib, ["zkhip"], [lib])
    for hasher in HASHERS:
        run_hasher(exe, M, hasher)
