"""Yardstick of the Poseidon tests (test_poseidon_*.py): a restatement of the reference's ethsnarks/poseidon/permutation.py over hashlib.blake2b
-- it reproduces the four constants and the hash that the reference pins as text (test/test_poseidon.py, src/test/test_poseidon.cpp) -- and a plain
width-w tree after ethsnarks/merkletree.py (unique() placeholders, proof() semantics).  Nothing here touches the library or its Python front end's
Poseidon code: ethsnarks_amd.gadgets is used for merkle_unique alone."""
import hashlib

from ethsnarks_amd import fields as F, gadgets as G
import merkle_cases as MC

R = F.FR
T, ROUNDS_F, ROUNDS_P = 6, 8, 57

# pinned by the reference
C0 = 14397397413755236225575615486459253198602422701513067526754101844196324375522
C64 = 10635360132728137321700090133109897687122647659471659996419791842933639708516
M00 = 19167410339349846567561662441069598364702008768579734801591448511131028229281
M55 = 20261355950827657195644012399234591122288573679402601053407151083849785332516
HASH_1_2 = 12242166908188651009877250812424843524687801523336557272219921456462821518061
# recorded from this restatement
HASH_0_0 = 951383894958571821976060584138905353883650994872035011055912076785884444545
HASH_4_RM1 = 20371162934311854307134494706805605308296023369376743919872286472089473906858
PINNED = [([1, 2], HASH_1_2), ([0, 0], HASH_0_0), ([R - 1] * 4, HASH_4_RM1)]


def _H(arg):
    if isinstance(arg, int):
        arg = arg.to_bytes(32, "little")
    return int.from_bytes(hashlib.blake2b(arg, digest_size=32).digest(), "little")


def _constants(seed, n):
    out = []
    for _ in range(n):
        seed = _H(seed)                                          # the chain runs on the unreduced digest
        out.append(seed % R)
    return out


C = _constants(b"poseidon_constants", ROUNDS_F + ROUNDS_P)
_c = _constants(b"poseidon_matrix_0000", 2 * T)
M = [[pow((_c[i] - _c[T + j]) % R, R - 2, R) for j in range(T)] for i in range(T)]


def poseidon(inputs, chained=False):
    assert len(inputs) > 0 and (chained or len(inputs) < T)
    state = list(inputs) + [0] * (T - len(inputs))
    for i, c in enumerate(C):
        state = [(v + c) % R for v in state]
        if i < ROUNDS_F // 2 or i >= ROUNDS_F // 2 + ROUNDS_P:
            state = [pow(v, 5, R) for v in state]
        else:
            state[0] = pow(state[0], 5, R)
        state = [sum(M[r][j] * v for j, v in enumerate(state)) % R for r in range(T)]
    return state if chained else state[0]


def _hash_chunk(nodes):
    return [poseidon(list(n)) for n in nodes]


def hash_nodes(nodes, pool=None):
    if pool is None or len(nodes) < 128:
        return _hash_chunk(nodes)
    step = max(32, (len(nodes) + 4 * MC.MAX_WORKERS - 1) // (4 * MC.MAX_WORKERS))
    out = []
    for part in pool.map(_hash_chunk, [nodes[i:i + step] for i in range(0, len(nodes), step)]):
        out.extend(part)
    return out


class PyTree:
    """levels[d] = the ceil(n / w^d) stored nodes of level d; anything else reads as the placeholder unique(d, index)"""

    def __init__(self, depth, width, leaves=(), pool=None):
        self.depth, self.width = depth, width
        self.levels = [list(leaves)] + [[] for _ in range(depth)]
        w = width
        for d in range(depth):
            cnt = len(self.levels[d])
            self.levels[d + 1] = hash_nodes([tuple(self.node(d, w * j + k) for k in range(w)) for j in range((cnt + w - 1) // w)], pool)

    def __len__(self):
        return len(self.levels[0])

    def node(self, d, o):
        return self.levels[d][o] if o < len(self.levels[d]) else G.merkle_unique(d, o)

    @property
    def root(self):
        return self.levels[self.depth][0] if len(self) else None

    def set(self, index, leaf):
        w = self.width
        self.levels[0][index] = leaf
        for d in range(self.depth):
            index //= w
            self.levels[d + 1][index] = poseidon([self.node(d, w * index + k) for k in range(w)])

    def digits(self, index):
        return [index // self.width ** d % self.width for d in range(self.depth)]

    def path(self, index):
        """merkletree.py:163-177: per level the node of the own parent without the own position; a single sibling is not wrapped in a list"""
        w, out = self.width, []
        for d in range(self.depth):
            start = index - index % w
            items = [self.node(d, o) for o in range(start, start + w) if o != index]
            out.append(items[0] if w == 2 else items)
            index //= w
        return out

    def placeholders(self, index):
        """[(level, [offsets of the absent siblings])] on the path of `index`"""
        w, out = self.width, []
        for d in range(self.depth):
            start = index - index % w
            holes = [o for o in range(start, start + w) if o != index and o >= len(self.levels[d])]
            if holes:
                out.append((d, holes))
            index //= w
        return out

    def verify(self, leaf, digits, path):
        item = leaf
        for digit, sibs in zip(digits, path):
            args = list(sibs) if isinstance(sibs, list) else [sibs]
            args.insert(digit, item)
            item = poseidon(args)
        return item == self.root


def assert_same_nodes(tree, ref):
    """every stored node of the device tree equals the Python tree's, and the absent nodes up to the end of the last parent are the placeholders"""
    w = ref.width
    assert len(tree) == len(ref)
    assert tree.root == ref.root
    for d in range(ref.depth + 1):
        cnt = len(ref.levels[d])
        for o in range(cnt):
            assert tree.leaf(d, o) == ref.levels[d][o], (d, o)
        for o in range(cnt, min(cnt + w - 1, w ** (ref.depth - d))):
            assert tree.leaf(d, o) == G.merkle_unique(d, o), (d, o)


def hash_cases(n_random, seed):
    """(inputs, expected) for every n_in = 1 .. 5 over the edge values {0, 1, r - 1} (every combination up to n_in = 3, all-equal and mixed rows
    above), and n_random random rows per n_in"""
    import itertools
    import random
    rng = random.Random(seed)
    edge = [0, 1, R - 1]
    by_n = {}
    for n_in in range(1, 6):
        rows = [list(t) for t in itertools.product(edge, repeat=n_in)] if n_in <= 3 else \
            [[e] * n_in for e in edge] + [[edge[(i + k) % 3] for i in range(n_in)] for k in range(3)]
        rows += [[rng.randrange(R) for _ in range(n_in)] for _ in range(n_random)]
        by_n[n_in] = rows
    return by_n


def ldot6_cases(p, loose, seed=9):
    """operand tuples (a0 .. a5, b0 .. b5) for Field::ldot6 in the style of arith_cases.tuple_cases: the a from the loose domain [0, 2p) (the
    strict one when not loose), the b canonical; edge, drawn, random and near-maximal tuples, and a = 2p - 1 (p - 1) in every slot with b = p - 1
    in every slot: the largest sum the precondition admits"""
    import random
    import arith_cases as K
    rng = random.Random(seed)
    ea, eb = K.edge_values(p, loose), K.edge_values(p, False)
    top = (2 * p if loose else p) - 1
    out = [(top,) * 6 + (p - 1,) * 6]
    out += [(a,) * 6 + (b,) * 6 for a in ea for b in eb[:6]]
    out += [tuple(rng.choice(ea) for _ in range(6)) + tuple(rng.choice(eb) for _ in range(6)) for _ in range(K.N_DRAWN)]
    out += [tuple(rng.randrange(top + 1) for _ in range(6)) + tuple(rng.randrange(p) for _ in range(6)) for _ in range(K.N_RANDOM)]
    for i in range(K.N_NEAR_MAX):
        out.append(tuple(top - rng.randrange(1 << (1 + i % 40)) for _ in range(6)) + tuple(p - 1 - rng.randrange(1 << (1 + i % 40)) for _ in range(6)))
    return out
