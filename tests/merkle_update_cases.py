"""Yardstick of the ordered-update tests (test_merkle_update_emul.py, test_merkle_update_gpu.py): the cases, and for each the reference that owes
nothing to the kernels under test -- the plain PyTree of merkle_cases.py / poseidon_cases.py updated with set() ONE update at a time, and the
witness of gadgets.merkle_update_circuit over ref.path(a_j) and ref.node(0, a_j) taken BEFORE update j.  Nothing here touches the library."""
import random
from collections import namedtuple

from ethsnarks_amd import gadgets as G, fields as F
import merkle_cases as MC
import poseidon_cases as PC

HASHERS = ("mimc", "poseidon")
STRIDE = {"mimc": 736, "poseidon": 322}

# depth, leaves of the tree before, the updates in order
Case = namedtuple("Case", "depth leaves indices values")
# the tree after, the k + 1 roots, per update the inputs of its circuit (ints, allocation order), {row: (r1cs, witness, roots)} of the rows asked for
Reference = namedtuple("Reference", "tree roots inputs circuits")


def n_supplied(hasher, D):
    """ONE, old_root, new_root, address bits, path, old_leaf, new_leaf (and the 29 IVs of the MiMC circuit): what a planner takes as known"""
    return 5 + 2 * D + (29 if hasher == "mimc" else 0)


def ref_tree(hasher, D, leaves, pool=None):
    return MC.PyTree(D, leaves, pool) if hasher == "mimc" else PC.PyTree(D, 2, leaves, pool)


def assert_same_nodes(hasher, tree, ref):
    (MC if hasher == "mimc" else PC).assert_same_nodes(tree, ref)


def shapes_case():
    """depth 3, 7 leaves: a repeated index (2), a sibling pair (2, 3), cousins (0 and 2, 3), self-sibling-self (2, 3, 2), index 6 whose sibling
    is the level-0 placeholder, and update 4, which writes the value leaf 0 already has: a no-op whose two roots are equal"""
    leaves = MC.random_leaves(7, 1201)
    values = MC.random_leaves(8, 1202)
    values[4] = leaves[0]
    return Case(3, leaves, [2, 3, 2, 6, 0, 2, 5, 3], values)


def single_case():
    return Case(3, MC.random_leaves(5, 1203), [4], MC.random_leaves(1, 1204))


def random_case(depth, n, k, seed):
    rng = random.Random(seed)
    return Case(depth, MC.random_leaves(n, seed), [rng.randrange(n) for _ in range(k)], MC.random_leaves(k, seed + 1))


def depth29_case():
    """5 rows x 29 levels x 2 sides = 290 lanes of the trace pass: five workgroups of 64, the last partial, rows that straddle workgroups"""
    return Case(29, MC.random_leaves(70, 1210), [0, 1, 0, 69, 64], MC.random_leaves(5, 1211))


def _circuit(args):
    """(witness, roots) of one update circuit: what crosses a process boundary"""
    _, w, roots = G.merkle_update_circuit(*args)
    return w, roots


def reference(hasher, case, rows=(), pool=None):
    """the PyTree chain of a case, and the gadget circuits of the given rows: circuits[j] = (r1cs, witness, roots), the constraint system (the
    same for every row) built once.  pool: a process pool for the tree build and for the witnesses when many rows are asked for"""
    D = case.depth
    ref = ref_tree(hasher, D, case.leaves, pool)
    ivs = MC.IVS if hasher == "mimc" else []
    roots, inputs, args = [ref.root], [], {}
    for j, (a, y) in enumerate(zip(case.indices, case.values)):
        old, path = ref.node(0, a), ref.path(a)
        ref.set(a, y)
        roots.append(ref.root)
        inputs.append([1, roots[j], roots[j + 1]] + [(a >> d) & 1 for d in range(D)] + path + [old, y] + list(ivs))
        if j in rows:
            args[j] = (D, hasher, old, y, a, path)
    circuits = {}
    if args:
        first = min(args)
        r1cs = G.merkle_update_circuit(*args[first])[0]
        order = sorted(args)
        done = pool.map(_circuit, [args[j] for j in order], chunksize=2) if pool is not None and len(order) > 4 else map(_circuit, [args[j] for j in order])
        for j, (w, rr) in zip(order, done):
            assert rr == (roots[j], roots[j + 1]) and w[:n_supplied(hasher, D)] == inputs[j] and len(w) == r1cs.V + 1
            circuits[j] = (r1cs, w, rr)
    return Reference(ref, roots, inputs, circuits)
