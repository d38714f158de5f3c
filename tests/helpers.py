"""shared helpers for the parity tests"""
import json
import os
import numpy as np
from ethsnarks_amd import r1cs as R, fields as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    with open(os.path.join(GOLDEN, "proofs_pyref.json")) as f:
        return json.load(f)


def build_case(case):
    if case["kind"] == "chain":
        r, w = R.synthetic_chain(case["nC"], case["nIn"], case["seed"])
    else:
        r, w = R.random_r1cs(case["nC"], case["nIn"], seed=case["seed"], small_values=case["small_values"])
    toxic = [int(t, 16) for t in case["toxic"]]
    return r, w, toxic


def rand_scalars(n, seed, ones_every=0, zeros_every=0):
    rng = R.SplitMix64(seed)
    sc = [rng.fr() for _ in range(n)]
    if ones_every:
        for i in range(0, n, ones_every):
            sc[i] = 1
    if zeros_every:
        for i in range(1, n, zeros_every):
            sc[i] = 0
    return sc


def structured_ntt_vectors(logm, seed=5):
    """[(label, (m, 4) limb array)]: transform inputs in which whole butterfly layers produce exact zeros and sums that equal the modulus
    -- a difference of equal elements comes out as 0 or as the second representative r of zero, and the last pass must store the canonical
    one.  The limbs are raw values below r (r - 1 is the largest valid representative)."""
    m = 1 << logm
    top, one, zero = F.ints_to_limbs([F.FR - 1])[0], F.ints_to_limbs([1])[0], np.zeros(4, dtype=np.uint64)
    const = lambda v: np.broadcast_to(v, (m, 4)).copy()
    delta0 = const(zero); delta0[0] = one
    delta_last = const(zero); delta_last[m - 1] = one
    alt = const(top); alt[1::2] = one
    rng = np.random.default_rng(seed + logm)
    mixed = rng.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64)
    mixed[:, 3] &= (1 << 59) - 1
    mixed[::9] = top; mixed[::8] = zero
    return [("zero", const(zero)), ("constant r-1", const(top)), ("delta at 0", delta0), ("delta at m-1", delta_last),
            ("alternating r-1, 1", alt), ("random with zeros and r-1", mixed)]


def tiled_bases(oracle, n, g2=False, distinct=512, seed=11):
    """n valid curve points: `distinct` oracle-generated multiples of the generator, tiled."""
    rng = R.SplitMix64(seed)
    d = min(n, distinct)
    if d == 0:
        return np.zeros((0, 16 if g2 else 8), dtype=np.uint64)
    pts = oracle.batch_mul(F.fr_to_mont([rng.fr() for _ in range(d)]), g2=g2)
    reps = (n + d - 1) // d
    return np.tile(pts, (reps, 1))[:n].copy()


def wide_sum_circuit(rows, width, pool=None, values=None, seed=1):
    """`rows` constraints (x_1 + ... + x_width) * ONE = x_new over fresh variables: every free variable sits in the A-query and every
    output in the C-query, so each of the V = rows * (width + 1) witness variables has a non-zero L base, and the L-query is much larger
    than the domain (m ~ rows).  The free variables take `values` (a list of rows * width ints) if given, else draws from a pool of
    `pool` random values (pool=None: every value drawn afresh) -- the pool size sets how many buckets the L digits fall into.
    Variable 1 (the first free variable) is the one public input.  Returns (R1CS, witness ints [V + 1])."""
    nfree = rows * width
    V = rows * (width + 1)
    rng = R.SplitMix64(seed)
    if values is None:
        if pool is None:
            values = [rng.fr() for _ in range(nfree)]
        else:
            vals = [rng.fr() for _ in range(pool)]
            values = [vals[rng.next() % pool] for _ in range(nfree)]
    assert len(values) == nfree
    w = [1]
    for j in range(rows):
        row = [int(v) % F.FR for v in values[j * width:(j + 1) * width]]
        w += row
        w.append(sum(row) % F.FR)
    j = np.arange(rows, dtype=np.int64)
    a_ptr = (j * width).tolist() + [nfree]
    a_col = (1 + np.arange(nfree, dtype=np.int64) + np.arange(nfree, dtype=np.int64) // width).astype(np.uint32)   # skips each row's output
    one = lambda n: np.broadcast_to(F.FR_ONE_MONT, (n, 4)).copy()
    ptr = lambda p: np.asarray(p, dtype=np.uint32)
    A = R.CSR(ptr(a_ptr), a_col, one(nfree))
    B = R.CSR(ptr(np.arange(rows + 1)), np.zeros(rows, dtype=np.uint32), one(rows))
    C = R.CSR(ptr(np.arange(rows + 1)), ((j + 1) * (width + 1)).astype(np.uint32), one(rows))
    return R.R1CS(rows, 1, V, A, B, C), w


# ---- the bucket bookkeeping of the MSM (ethsnarks_amd/csrc/msm.hpp, msm_impl.hpp) restated in Python: tests that target the heavy-bucket
# path check with it that their inputs really reach it, so that a later change of shapes or knobs cannot quietly turn them into easy cases
MSM_HEAVY = 64


def msm_digit_counts(scalars, c, plog=0):
    """entries per bucket of the signed c-bit digit sort (msm_digit, k_sort_count) of one proof: scalars are canonical ints; window w adds
    its digit d to bucket (w mod 2^plog) * 2^(c-1) + |d| - 1 (plog > 0: the bucket planes of frugal tables).  Equal scalars are counted once."""
    from collections import Counter
    nbp, full, W, S = 1 << (c - 1), 1 << c, 254 // c + 1, 1 << plog
    cnt = np.zeros(nbp * S, dtype=np.int64)
    for s, mult in Counter(int(s) for s in scalars).items():
        carry = 0
        for w in range(W):
            d = ((s >> (w * c)) & (full - 1)) + carry
            carry = 0
            if d > nbp:
                d, carry = full - d, 1
            if d:
                cnt[(w & (S - 1)) * nbp + d - 1] += mult
    return cnt


def digit_pool(P, c, windows):
    """P scalars whose signed c-bit digits are all positive and pairwise distinct across (scalar, window): every (value, window) pair owns a
    bucket (no carries; the lowest `windows` windows only, below 254 bits, so that the values stay below r)"""
    assert P * windows < 1 << (c - 1) and c * windows <= 253
    return [sum((j * windows + w + 1) << (c * w) for w in range(windows)) for j in range(P)]


class ChunkRule:
    """msm.hpp ChunkRule: one chunk length for the whole entry list, from the slot count and [seg_min, seg_max]"""

    def __init__(self, slots, seg_min, seg_max):
        self.slots, self.seg_min, self.seg_max = slots, seg_min, seg_max

    def len(self, total):
        if self.seg_min * self.slots >= total:
            return self.seg_min
        per_round = self.seg_max * self.slots
        lanes = -(-total // per_round) * self.slots
        return max(-(-total // lanes), self.seg_min)

    def max_chunks(self, entries_bound):
        return entries_bound // self.seg_max + self.slots + 1

    @staticmethod
    def of_shape(n, c, machine_threads, batch=1, waves=(4, 3), env=os.environ):
        """MsmShape::set + set_slots for a G1 MSM of n scalars (waves: G1's WAVES_PER_SIMD, WAVES_PER_SIMD_PAIRS); machine_threads(w) is
        msm_machine_threads -- 32 w in the CPU emulation, CUs x 4 x w x 64 on a device"""
        W = 254 // c + 1
        total = n * W * batch
        quad_acc = 4 if total <= 1 << 17 else 1
        if "ZK_MSM_QUAD_ACC" in env:
            quad_acc = 4 if int(env["ZK_MSM_QUAD_ACC"]) else 1
        pairs = total >= 3 << 21
        if "ZK_ACC_PAIRS" in env:
            pairs = int(env["ZK_ACC_PAIRS"]) != 0
        seg_min, seg_max = (8 if total <= 1 << 23 else 32), 48
        if int(env.get("ZK_SEG_MIN", "0")) >= 4:
            seg_min = int(env["ZK_SEG_MIN"])
        if int(env.get("ZK_SEG_MAX", "0")) >= 4:
            seg_max = int(env["ZK_SEG_MAX"])
        seg_max = max(seg_max, seg_min)
        return ChunkRule(max(machine_threads(waves[1] if pairs else waves[0]) // quad_acc, 1), seg_min, seg_max)


def bucket_pieces(counts, rule):
    """chunk pieces per bucket (msm_piece_range) of a sort with these per-bucket entry counts"""
    off = np.concatenate([[0], np.cumsum(counts)])
    seg = rule.len(int(off[-1]))
    e0, e1 = off[:-1], off[1:]
    return np.where(e1 > e0, (np.maximum(e1, 1) - 1) // seg - e0 // seg + 1, 0)


def old_heavy_capacity(n_h, c, rule_h, sets=1):
    """heavy-list entries MsmWork::alloc gave an MSM of n_h scalars before the list was sized for every bucket: n_pieces / MSM_HEAVY + 2"""
    W, nb = 254 // c + 1, 1 << (c - 1)
    return (rule_h.max_chunks(n_h * W * sets) + nb * sets + 1) // MSM_HEAVY + 2
