"""Inputs for the two probes of the H pipeline (include/zkhip.h): zk_ntt_probe -- ONE call of the transform driver ntt_run (csrc/ntt.hpp) with
the batch, stride and fused steps a proof gives it -- and zk_ctx_probe_h -- the H pipeline of a batch, step by step.  Pure Python / numpy.

Transform cases.  ntt_run does the first NTT_TILE_LOG = 11 stages in one pass and the rest in ceil(rest / 9) passes of equal length; inside
a pass, stages go in pairs with an odd one last.  The sizes are those at which another path is taken:
    logm 0         the k == 0 tile: scaling only
    1, 2, 3        k < 2 unfused load; a single pair; a pair plus an odd stage
    10, 11         one pass, even and odd stage count
    12             a second pass with k = 1: unfused load, radix-2 tail, 2^10 columns
    13, 14         a second pass with k = 2 (memory to memory) and k = 3
    21             three passes, 11 + 5 + 5 (device runner only)
passes() restates that plan and every case asserts the path it is there for.  The combinations are the three calls a proof makes
(enqueue_compute_h, enqueue_h_from_chains in csrc/zkhip.cpp), the four of zk_ntt at batch > 1, and one with every fused step at once; the
three-polynomial call runs with alt_from in {0, 1, batch - 1, batch, 0xffffffff}; batches are 1, 2, 3 and 5.  Every vector of a batch, and
its in2 and sub, holds other data; every second case has stride = m + 5 with a sentinel in the gaps.  Input words are canonical except in
the "loose" cases: the batched forward transform with nothing fused, at 2^0, 2^1, a one-pass and a two-pass size, whose inputs hold words
r + x, so that only the canonicalisation of the last pass brings the output back below r (loose_words()).

H-pipeline systems: random satisfiable systems (r1cs.random_r1cs) with domains 256 (below one k_hl_product workgroup), 2 048 (exactly one,
one transform pass) and 4 096 (two workgroups, two passes); three witnesses each, and the middle one perturbed in a free variable."""
import functools
from collections import namedtuple
import numpy as np
from ethsnarks_amd import r1cs as R, fields as F
from helpers import structured_ntt_vectors

TILE_LOG, MIN_LOGC = 11, 2                       # NTT_TILE_LOG, NTT_MIN_LOGC of csrc/ntt.hpp
POSTS = ("none", "inv_m", "icoset", "inv_then_coset", "inv_m_zinv", "icoset_zinv")
SENTINEL = 0xA5C3F00DDEADBEEF                    # every limb of the output before the call
NO_ALT = 0xffffffff

NttCase = namedtuple("NttCase", "name logm batch stride inverse pre post post_alt alt_from in2 sub data seed")


def passes(logm):
    """[(s0, k, logc)] of ntt_run for this size"""
    if logm == 0:
        return [(0, 0, 0)]
    k0 = min(logm, TILE_LOG)
    out, rem, kmax, s0 = [(0, k0, 0)], logm - k0, TILE_LOG - MIN_LOGC, k0
    npass = (rem + kmax - 1) // kmax
    while rem:
        k = (rem + npass - 1) // npass
        out.append((s0, k, min(TILE_LOG - k, s0)))
        rem -= k; npass -= 1; s0 += k
    return out


PLAN = {0: [(0, 0, 0)], 1: [(0, 1, 0)], 2: [(0, 2, 0)], 3: [(0, 3, 0)], 10: [(0, 10, 0)], 11: [(0, 11, 0)], 12: [(0, 11, 0), (11, 1, 10)],
        13: [(0, 11, 0), (11, 2, 9)], 14: [(0, 11, 0), (11, 3, 8)], 21: [(0, 11, 0), (11, 5, 6), (16, 5, 6)]}
for _l, _p in PLAN.items():
    assert passes(_l) == _p, (_l, passes(_l))
SMALL, LARGE, DEVICE_ONLY = (0, 1, 2, 3), (10, 11, 12, 13, 14), (21,)
LOOSE_SIZES = (0, 1, 10, 12)                     # scaling only, one stage, one pass, two passes

#          name: (inverse, pre, post, post_alt, in2, sub)
COMBOS = {"abc_inverse": (True, "none", "inv_then_coset", "inv_m_zinv", False, False),      # enqueue_compute_h: iFFT of A, B and C
          "to_coset": (False, "none", "none", "none", False, False),                        # ... FFT of A, B: nothing fused, canonicalised
          "h_last": (True, "none", "icoset_zinv", "none", True, True),                      # ... icosetFFT of A B, - C / Z(g)
          "fwd_coset": (False, "coset_fwd", "none", "none", False, False),                  # zk_ntt's other three
          "inv": (True, "none", "inv_m", "none", False, False),
          "inv_coset": (True, "none", "icoset", "none", False, False),
          "everything": (True, "coset_fwd", "icoset", "inv_m_zinv", True, True)}


def _build():
    cases = {}

    def add(logm, combo, batch, alt_from=NO_ALT, data="random"):
        inverse, pre, post, post_alt, in2, sub = COMBOS[combo]
        alt = {NO_ALT: "none"}.get(alt_from, str(alt_from))
        name = "l%d_%s_b%d_alt%s%s" % (logm, combo, batch, alt, "" if data == "random" else "_" + data)
        if name in cases:
            return
        m = 1 << logm
        stride = m + 5 if len(cases) % 2 else m
        cases[name] = NttCase(name, logm, batch, stride, inverse, pre, post, post_alt, alt_from, in2, sub, data, 1000 + len(cases))

    for logm in SMALL + LARGE:
        small = logm in SMALL
        for batch in (1, 2, 3, 5) if small else (3,):
            for alt_from in (0, 1, batch - 1, batch, NO_ALT):
                add(logm, "abc_inverse", batch, alt_from)
        if not small:
            add(logm, "abc_inverse", 1, 0); add(logm, "abc_inverse", 1, 1); add(logm, "abc_inverse", 2, 1); add(logm, "abc_inverse", 5, 4)
        add(logm, "abc_inverse", 3, 2, "structured")
        for batch in (1, 2, 3, 5) if small else (1, 3):
            add(logm, "h_last", batch)
        add(logm, "h_last", 3, data="structured")
        for batch in (1, 2, 3, 5) if small else (2,):
            add(logm, "to_coset", batch)
        add(logm, "to_coset", 5, data="structured")                  # structured vectors 0 .. 4
        add(logm, "to_coset", 3, data="structured")                  # ... and 3 .. 5 (structured(): a batch of three starts at 3)
        for combo in ("fwd_coset", "inv", "inv_coset"):
            for batch in (2, 3, 5) if small else (2,):
                add(logm, combo, batch)
        add(logm, "everything", 2, 1)
        add(logm, "everything", 5, 4, "structured")
    for logm in DEVICE_ONLY:                                         # 64 MiB per vector: two cases, batch = 2, alt_from = 1
        add(logm, "everything", 2, 1)
        add(logm, "to_coset", 2, data="structured")
    for logm in LOOSE_SIZES:                                         # input words r + x: only the last pass's Fr::canon reduces what they leave
        for batch in (2, 3):
            add(logm, "to_coset", batch, data="loose")
    return cases


NTT_CASES = _build()
EMUL_NTT_CASES = tuple(n for n, c in NTT_CASES.items() if c.logm < 15)
for _logm in SMALL + LARGE:
    _mine = [c for c in NTT_CASES.values() if c.logm == _logm]
    assert {c.batch for c in _mine} >= {1, 2, 3, 5}
    assert {(c.batch, c.alt_from) for c in _mine if c.batch == 3 and c.post_alt != "none"} >= {(3, 0), (3, 1), (3, 2), (3, 3), (3, NO_ALT)}
    assert any(c.stride > (1 << _logm) for c in _mine) and any(c.stride == (1 << _logm) and c.batch > 1 for c in _mine)
    assert any(c.data == "structured" and c.post == "none" and not c.inverse for c in _mine)
assert all(c.batch == 2 and c.logm == 21 for n, c in NTT_CASES.items() if n not in EMUL_NTT_CASES)


def _random(rng, shape):
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 59) - 1)                            # below 2^251 < r: canonical words
    return a


def loose_words(logm):
    """how many leading words of every vector of a "loose" case are r + x, the second representative of x < 2^251 (the butterflies accept
    [0, 2r): csrc/bn254.hpp "loose domain").  Up to one stage: all of them.  Beyond: word 0 alone -- it is never a subtrahend and never
    multiplied (the first operand of every butterfly it meets), which also keeps the CPU stand-in, whose loose operations are the strict
    ones and add r where the device adds 2r, inside its range.  On the device every output carries it through sums that fold at 2r only;
    the stand-in's strict sums reduce on the way, so there the sizes 2^0 and 2^1 are the ones that need the last pass's reduction."""
    return 1 << logm if logm <= 1 else 1


def add_modulus(a):
    """a + r limb by limb; a: (..., 4) u64 words below 2^251, so nothing leaves 256 bits"""
    out, carry = np.empty_like(a), np.zeros(a.shape[:-1], dtype=np.uint64)
    for l in range(4):
        rl = np.uint64((F.FR >> (64 * l)) & 0xFFFFFFFFFFFFFFFF)
        s = a[..., l] + rl
        c1 = s < rl
        s2 = s + carry
        carry = (c1 | (s2 < s)).astype(np.uint64)
        out[..., l] = s2
    assert not carry.any()
    return out


def _structured(logm, batch, rotate):
    vs = [v for _, v in structured_ntt_vectors(logm)]
    first = 3 if batch == 3 else 0
    return np.stack([vs[(first + rotate + v) % len(vs)] for v in range(batch)])


def ntt_inputs(case):
    """(in, in2 | None, sub | None, out before the call): (batch, stride, 4) u64 each, seeded; the gaps of the inputs hold random words, the
    whole of `out` the sentinel"""
    m, shape = 1 << case.logm, (case.batch, case.stride)
    rng = np.random.default_rng(case.seed)
    arrays = []
    for i, wanted in enumerate((True, case.in2, case.sub)):
        if not wanted:
            arrays.append(None)
            continue
        a = _random(rng, shape)
        if case.data == "structured":
            a[:, :m] = _structured(case.logm, case.batch, 2 * i)     # in, in2 and sub of a vector are three different structured vectors
        if case.data == "loose" and i == 0:
            a[:, :loose_words(case.logm)] = add_modulus(a[:, :loose_words(case.logm)])
        arrays.append(a)
    out = np.full(shape + (4,), SENTINEL, dtype=np.uint64)
    return arrays[0], arrays[1], arrays[2], out


# ---------------------------------------------------------------- systems for the H probe
#           name: (nC, nIn, seed)
SYSTEMS = {"m256": (200, 3, 71), "m2048": (2040, 5, 72), "m4096": (3000, 2, 73)}
DOMAIN = {"m256": 256, "m2048": 2048, "m4096": 4096}
GRID = {"m256": 1, "m2048": 1, "m4096": 2}                           # workgroups of k_hl_product: one pair of sums per 2 048 elements
WITNESS_SEEDS = {"a": 501, "b": 502, "c": 503}
BAD_SEED = 502                                                       # the perturbed witness is "b" with one free variable changed

HSystem = namedtuple("HSystem", "r1cs rows_a rows_b rows_c witnesses free")


@functools.lru_cache(maxsize=None)
def system(name):
    """-> HSystem; witnesses: {"a", "b", "c": satisfying, "bad": "b" with the free variable nIn + 1 increased by one, not re-solved}"""
    nC, nIn, seed = SYSTEMS[name]
    ws, r = {}, None
    for label, wseed in WITNESS_SEEDS.items():
        r, ws[label] = R.random_r1cs(nC, nIn, seed=seed, witness_seed=wseed)
    free = nIn + 1                                                   # variables 1 .. nIn + 2 are free; this one is no public input
    bad = list(ws["b"]); bad[free] = (bad[free] + 1) % F.FR
    ws["bad"] = bad
    assert r.domain_size == DOMAIN[name] and -(-r.domain_size // 2048) == GRID[name]
    assert len({tuple(w) for w in ws.values()}) == 4
    for label in WITNESS_SEEDS:
        assert r.is_satisfied(ws[label]), (name, label)
    assert not r.is_satisfied(bad), name
    assert any(i == free for row in r.A.to_rows() + r.B.to_rows() for i, _ in row), "the perturbed variable stands in no row"
    return HSystem(r, r.A.to_rows(), r.B.to_rows(), r.C.to_rows(), ws, free)


BATCHES = {"k1": ("a",), "k3": ("a", "b", "c"), "k3_bad_middle": ("a", "bad", "c")}
