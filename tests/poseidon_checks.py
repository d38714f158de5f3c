"""What the Poseidon tests assert on both builds, shared by test_poseidon_emul.py and test_poseidon_gpu.py: every check takes the binding (the
merkle module or the prover module with the emulation or the device library loaded) and compares with poseidon_cases.py.  Exact comparisons."""
from ethsnarks_amd import fields as F, gadgets as G
import arith_ref as A
import poseidon_cases as PC

LDOT6 = 25                                                         # the probe index of ldot6 in the Fr and Fq groups (include/zkhip.h)


def check_constants(M):
    c, m = M.poseidon_constants()
    assert c == PC.C and m == PC.M
    assert c[0] == PC.C0 and c[64] == PC.C64 and m[0][0] == PC.M00 and m[5][5] == PC.M55
    assert G.poseidon_constants() == (PC.C, PC.M)


def check_hashing(M, n_random):
    for inputs, want in PC.PINNED:
        assert PC.poseidon(inputs) == want
        assert M.poseidon_hash([inputs]) == [want], inputs
    for n_in, rows in PC.hash_cases(n_random, 5).items():
        assert M.poseidon_hash(rows) == [PC.poseidon(r) for r in rows], n_in


def check_permute(M, n_random):
    import random
    rng = random.Random(6)
    states = [[0] * 6, [F.FR - 1] * 6, [1, 2, 0, 0, 0, 0]] + [[rng.randrange(F.FR) for _ in range(6)] for _ in range(n_random)]
    once = M.poseidon_permute(states)
    assert once == [PC.poseidon(s, chained=True) for s in states]
    assert once[2][0] == PC.HASH_1_2
    assert M.poseidon_permute(once) == [PC.poseidon(s, chained=True) for s in once]


def check_ldot6(zk, field, loose, extra_random=0):
    """the raw result is congruent to sum a_i b_i / R and lies in [0, 2p) ([0, p) for the strict emulation form)"""
    import random
    p = A.MOD[field]
    op = (zk.PROBE_FR if field == "fr" else zk.PROBE_FQ) + LDOT6
    assert zk.arith_probe_shape(op) == (12, 1)
    cases = PC.ldot6_cases(p, loose)
    rng = random.Random(77)
    top = 2 * p if loose else p
    cases += [tuple(rng.randrange(top) for _ in range(6)) + tuple(rng.randrange(p) for _ in range(6)) for _ in range(extra_random)]
    assert cases[0] == ((2 * p - 1 if loose else p - 1),) * 6 + (p - 1,) * 6
    n = len(cases)
    out = zk.arith_probe(op, F.ints_to_limbs([v for t in cases for v in t]).reshape(n, 12, 4))
    got = F.limbs_to_ints(out.reshape(n, 4))
    rinv = pow(1 << 256, p - 2, p)
    bad = []
    for i, (t, g) in enumerate(zip(cases, got)):
        want = sum(a * b for a, b in zip(t[:6], t[6:])) * rinv % p
        if g % p != want or g >= top:
            bad.append("ldot6 %s case %d: got 0x%x, want 0x%x (mod p) below %s" % (field, i, g, want, "2p" if loose else "p"))
    assert not bad, "%d of %d cases fail, the first:\n  " % (len(bad), n) + "\n  ".join(bad[:5])
