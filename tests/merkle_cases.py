"""Yardstick of the Merkle tree tests (test_merkle_emul.py, test_merkle_gpu.py): a plain level-by-level tree over gadgets.mimc_hash, which the
gadget tests pin to the reference's MiMC vectors, and the reference's known answers (test/test_merkle.py).  Nothing here touches the library."""
import os
from concurrent.futures import ProcessPoolExecutor

from ethsnarks_amd import gadgets as G, fields as F, r1cs as R

ITEM_A = 3703141493535563179657531719960160174296085208671919316200479060314459804651
ITEM_B = 134551314051432487569247388144051420116740427803855572138106146683954151557
KNOWN1_ROOT = 3075442268020138823380831368198734873612490112867968717790651410945045657947
KNOWN29_ROOT_ONE = 5635502254919888512883611961327385811173415612631829359029947885796109426800
KNOWN29_ROOT_TWO = 14972246236048249827985830600768475898195156734731557762844426864943654467818
KNOWN29_NODES = {
    (0, 0): ITEM_A,
    (1, 0): 3075442268020138823380831368198734873612490112867968717790651410945045657947,
    (2, 0): 10399465128272526817755257959020023025563587559350936053132523411421423507430,
    (1, 1): 17296471688945713021042054900108821045192859417413320566181654591511652308323,
    (2, 1): 4832852105446597958495745596582249246190817345027389430471458078394903639834,
    (13, 1): 14116139569958633576637617144876714429777518811711593939929091541932333542283,
    (22, 1): 16077039334695461958102978289003547153551663194787878097275872631374489043531,
}
UNIQUES = {
    (20, 20): 6738165491478210350639451800403024427867073896603076888955948358229240057870,
    (2, 2): 21534879888322772601810176771999178940739467644392123609236489175629034941722,
    (0, 0): 2544023609834722662089612003212769975105508295482723304413974529614913939747,
}
IVS = G.merkle_ivs(29)
MAX_WORKERS = 16


def _hash_chunk(args):
    pairs, iv = args
    return [G.mimc_hash([l, r], iv) for l, r in pairs]


def hash_pairs(pairs, iv, pool=None):
    """[mimc_hash([l, r], iv)]; over a process pool when one is given and the list is long"""
    if pool is None or len(pairs) < 256:
        return _hash_chunk((pairs, iv))
    step = max(64, (len(pairs) + 4 * MAX_WORKERS - 1) // (4 * MAX_WORKERS))
    out = []
    for part in pool.map(_hash_chunk, [(pairs[i:i + step], iv) for i in range(0, len(pairs), step)]):
        out.extend(part)
    return out


def make_pool():
    return ProcessPoolExecutor(max_workers=min(MAX_WORKERS, os.cpu_count() or 1))


class PyTree:
    """levels[d] = the ceil(n / 2^d) stored nodes of level d; anything else is the placeholder merkle_unique(d, index)"""

    def __init__(self, depth, leaves=(), pool=None):
        self.depth = depth
        self.levels = [list(leaves)] + [[] for _ in range(depth)]
        self._rebuild(pool)

    def _rebuild(self, pool=None):
        for d in range(self.depth):
            cur = self.levels[d]
            pairs = [(cur[2 * j], cur[2 * j + 1] if 2 * j + 1 < len(cur) else G.merkle_unique(d, 2 * j + 1)) for j in range((len(cur) + 1) // 2)]
            self.levels[d + 1] = hash_pairs(pairs, IVS[d], pool)

    def __len__(self):
        return len(self.levels[0])

    def node(self, d, o):
        return self.levels[d][o] if o < len(self.levels[d]) else G.merkle_unique(d, o)

    @property
    def root(self):
        return self.levels[self.depth][0] if len(self) else None

    def set(self, index, leaf):
        self.levels[0][index] = leaf
        for d in range(self.depth):
            index >>= 1
            self.levels[d + 1][index] = G.mimc_hash([self.node(d, 2 * index), self.node(d, 2 * index + 1)], IVS[d])

    def path(self, index):
        return [self.node(d, (index >> d) ^ 1) for d in range(self.depth)]

    def bits(self, index):
        return [(index >> d) & 1 for d in range(self.depth)]

    def placeholder_levels(self, index):
        """the levels on which the path of `index` holds a placeholder"""
        return [d for d in range(self.depth) if ((index >> d) ^ 1) >= len(self.levels[d])]


def random_leaves(n, seed):
    rng = R.SplitMix64(seed)
    return [rng.fr() for _ in range(n)]


def assert_same_nodes(tree, ref):
    """every stored node of the device tree equals the Python tree's, and the first absent node of every level is the placeholder"""
    assert len(tree) == len(ref)
    assert tree.root == ref.root
    for d in range(ref.depth + 1):
        cnt = len(ref.levels[d])
        for o in range(cnt):
            assert tree.leaf(d, o) == ref.levels[d][o], (d, o)
        if cnt < (1 << (ref.depth - d)):
            assert tree.leaf(d, cnt) == G.merkle_unique(d, cnt), (d, cnt)
