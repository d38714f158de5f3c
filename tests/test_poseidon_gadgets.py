"""The Poseidon front end of ethsnarks_amd/gadgets.py -- poseidon(), FifthPowerGadget, PoseidonGadget = Poseidon128<nInputs, nOutputs>, the
membership and preimage circuits -- against the restatement of the reference's permutation and tree in poseidon_cases.py.  Host code only."""
import pytest
from ethsnarks_amd import gadgets as G, fields as F
import merkle_cases as MC
import poseidon_cases as PC


def test_native_poseidon_equals_the_restatement():
    assert G.poseidon_constants() == (PC.C, PC.M)
    for inputs, want in PC.PINNED:
        assert G.poseidon(inputs) == want
    for n_in, rows in PC.hash_cases(3, 21).items():
        assert [G.poseidon(r) for r in rows] == [PC.poseidon(r) for r in rows], n_in
    s = [5, 4, 3, 2, 1, 0]
    assert G.poseidon(s, chained=True) == PC.poseidon(s, chained=True)


def gadget(inputs, n_outputs=1):
    pb = G.Protoboard()
    vars_ = pb.allocate_array(len(inputs), inputs)
    before = len(pb.values)
    g = G.PoseidonGadget(pb, vars_, n_outputs)
    g.generate_r1cs_witness()
    g.generate_r1cs_constraints()
    return pb, g, len(pb.values) - before


def test_poseidon_gadget_2_1():
    pb, g, new_vars = gadget([1, 2])
    assert pb.num_constraints() == 316 and new_vars == 315 + 1
    assert pb.is_satisfied() and pb.val(g.result()) == PC.HASH_1_2
    # allocation order: x2, x4, x5 per S-box in round order, the output variable last
    first = g.rounds[0].sboxes[0]
    assert (first.x2, first.x4, first.x5) == (3, 4, 5) and g.outputs == [3 + 315]
    assert [len(r.sboxes) for r in g.rounds] == [6] * 4 + [1] * 57 + [6] * 4
    assert pb.val(first.x5) == pow(1 + PC.C[0], 5, F.FR)
    third = g.rounds[0].sboxes[2]                                  # beyond nInputs: the constant alone is raised
    assert pb.val(third.x5) == pow(PC.C[0], 5, F.FR)
    assert pb.A[6] == {0: PC.C[0]} and pb.B[6] == {0: PC.C[0]} and pb.C[6] == {third.x2: 1}
    # a partial round's state elements are linear combinations that grow: ONE, every S-box output since the last full round
    assert len(g.rounds[5].state[1]) == 1 + 6 + 1 and len(g.rounds[60].state[1]) == 1 + 6 + 56
    # in solved order: every constraint introduces exactly one new variable, alone in C (the closing ones: the output)
    known = set(range(3))
    for a, b, c in zip(pb.A, pb.B, pb.C):
        assert set(a) <= known and set(b) <= known and len(c) == 1 and not set(c) <= known
        known |= set(c)
    mid = g.rounds[30].sboxes[0].x4
    pb.set_val(mid, pb.val(mid) + 1)                               # one S-box variable altered
    assert not pb.is_satisfied()


@pytest.mark.parametrize("inputs,n_outputs", [([7, 8, 9], 2), ([F.FR - 1], 1), ([0, 0, 0, 0, 0], 6)])
def test_poseidon_gadget_other_shapes(inputs, n_outputs):
    pb, g, new_vars = gadget(inputs, n_outputs)
    assert pb.is_satisfied()
    assert new_vars == 315 + n_outputs and pb.num_constraints() == 315 + n_outputs
    assert [pb.val(o) for o in g.outputs] == PC.poseidon(inputs + [0] * (6 - len(inputs)), chained=True)[:n_outputs]
    assert pb.val(g.result()) == PC.poseidon(inputs)


def test_membership_circuit_depth_3():
    leaves = MC.random_leaves(6, 71)
    ref = PC.PyTree(3, 2, leaves)
    for i in (0, 5):                                               # 5: a placeholder on level 1
        r, w, root = G.poseidon_membership_circuit(3, leaf=leaves[i], address=i, path=ref.path(i))
        assert r.nC == 322 * 3 + 1 and r.nIn == 1 and root == ref.root == w[1]
        assert w[2:5] == ref.digits(i) and w[5:8] == ref.path(i) and w[8] == leaves[i]
        assert r.is_satisfied(w)
    r29 = G.poseidon_membership_circuit(29)[0]
    assert r29.nC == 9339 and r29.domain_size == 1 << 14


def test_preimage_circuit():
    r, w, digest = G.poseidon_preimage_circuit(2)
    assert r.nC == 317 and r.nIn == 1 and w[1] == digest == PC.poseidon(w[2:4])
    r4, w4, d4 = G.poseidon_preimage_circuit(4)
    assert d4 == PC.poseidon(w4[2:6]) and r4.nC == 317
