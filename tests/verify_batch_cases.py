"""shared material of test_verify_batch_emul.py / test_verify_batch_gpu.py: proofs as integers, tampered variants whose points stay in
their groups (so that only the pairing equation can reject them), ill-formed variants, and the mapping of the device tower to pyref's
polynomial basis.  `zk` is the binding (ethsnarks_amd.prover) with the library under test loaded."""
import json
import pyref
from ethsnarks_amd import r1cs as R, fields as F

Q, RR = pyref.Q, pyref.R
BN_Z = 4965661367192848881
FE_CHAIN_POWER = 2 * BN_Z * (6 * BN_Z * BN_Z + 3 * BN_Z + 1)      # pairing.hpp: final_exp(f) = f^(FE_CHAIN_POWER (q^12 - 1) / r)


def parse(proof_json):
    d = json.loads(proof_json) if isinstance(proof_json, str) else proof_json
    return pyref.g1_from_json(d["A"]), pyref.g2_from_json(d["B"]), pyref.g1_from_json(d["C"]), [int(v, 16) for v in d["input"]]


def text(A, B, C, inputs):
    return pyref.proof_to_json(A, B, C, inputs)


def as_dict(proof_json):
    return json.loads(proof_json)


def g2_mul_raw(p, k):
    """[k]p on the twist WITHOUT reducing k mod r (pyref.g2_mul reduces, which is only right inside the subgroup)"""
    acc = None
    while k:
        if k & 1:
            acc = pyref.g2_add(acc, p)
        p = pyref.g2_add(p, p)
        k >>= 1
    return acc


def f2_sqrt(a):
    """a root of a in Fq2 = Fq[u]/(u^2 + 1), or None (q = 3 mod 4: complex method)"""
    if a == (0, 0):
        return (0, 0)
    a1 = pyref.f2_pow(a, (Q - 3) // 4)
    alpha = pyref.f2_mul(a1, pyref.f2_mul(a1, a))
    x0 = pyref.f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        x = pyref.f2_mul((0, 1), x0)
    else:
        b = pyref.f2_pow(pyref.f2_add((1, 0), alpha), (Q - 1) // 2)
        x = pyref.f2_mul(b, x0)
    return x if pyref.f2_mul(x, x) == a else None


def twist_point_outside_subgroup(seed):
    """a point of the twist y^2 = x^3 + 3/xi that is not in the order-r subgroup (the cofactor 2q - r makes a random point such a
    one with overwhelming probability; asserted)"""
    rng = R.SplitMix64(seed)
    while True:
        x = (rng.fr() % Q, rng.fr() % Q)
        y = f2_sqrt(pyref.f2_add(pyref.f2_mul(pyref.f2_mul(x, x), x), pyref.TWIST_B))
        if y is None:
            continue
        P = (x, y)
        assert pyref.g2_on_curve(P)
        assert g2_mul_raw(P, RR) is not None
        return P


# ---- tampered proofs that only the pairing equation rejects
def tamper_pairing(kind, proof_json):
    A, B, C, inp = parse(proof_json)
    if kind == "A2":
        A = pyref.g1_add(A, A)
    elif kind == "C+G":
        C = pyref.g1_add(C, pyref.G1_GEN)
    elif kind == "B+G2":
        B = pyref.g2_add(B, pyref.G2_GEN)
    elif kind == "input":
        inp = list(inp)
        if inp:
            inp[-1] = (inp[-1] + 1) % RR
        else:                                   # a key without inputs: move C instead
            C = pyref.g1_add(C, pyref.g1_add(pyref.G1_GEN, pyref.G1_GEN))
    else:
        raise ValueError(kind)
    return text(A, B, C, inp)


PAIRING_KINDS = ["A2", "C+G", "B+G2", "input"]


def swap_inputs(p1, p2):
    """two proofs of different witnesses with their inputs swapped"""
    A1, B1, C1, i1 = parse(p1)
    A2, B2, C2, i2 = parse(p2)
    return text(A1, B1, C1, i2), text(A2, B2, C2, i1)


# ---- ill-formed proofs
def tamper_form(kind, proof_json, seed=1):
    A, B, C, inp = parse(proof_json)
    if kind == "coord>=q":
        A = (A[0] + Q, A[1])
    elif kind == "input>=r":
        if not inp:
            return None
        inp = [inp[0] + RR] + list(inp[1:])
    elif kind == "A off curve":
        A = (A[0], (A[1] + 1) % Q)
    elif kind == "B outside subgroup":
        B = twist_point_outside_subgroup(seed)
    elif kind == "C off curve":
        C = ((C[0] + 1) % Q, C[1])
    elif kind == "B off twist":
        B = (B[0], ((B[1][0] + 1) % Q, B[1][1]))
    elif kind == "too few inputs":
        if not inp:
            return None
        inp = inp[:-1]
    elif kind == "too many inputs":
        inp = list(inp) + [5]
    elif kind == "not json":
        return "{ \"A\" : [\"0x1\"] }"
    else:
        raise ValueError(kind)
    return text(A, B, C, inp)


FORM_KINDS = ["coord>=q", "input>=r", "A off curve", "B outside subgroup", "C off curve", "B off twist", "too few inputs", "too many inputs", "not json"]


def interleave(valid, bad):
    """[valid, bad0, valid, bad1, ...]: with its rotation by one, every batch position sees both verdicts"""
    out = []
    for b in bad:
        out += [valid, b]
    return out


def expected(zk, vk_json, texts):
    """the host verifier's verdicts (zk_verify); a text it cannot parse is `not accepted`"""
    res = []
    for t in texts:
        try:
            res.append(zk.stub_verify(vk_json, t))
        except zk.ZkError as e:
            assert e.code == 3
            res.append(False)
    return res


# ---- tower <-> pyref's basis: coefficient a_ij of v^i w^j is entry 3 j + i of the 6 Fq2 values, at w^(2 i + j)
def tower_to_pyref(vals12):
    assert len(vals12) == 12
    return pyref._embed([(2 * i + j, (vals12[2 * (3 * j + i)], vals12[2 * (3 * j + i) + 1])) for j in range(2) for i in range(3)])


def tower_random(rng):
    return [rng.fr() % Q for _ in range(12)]


def tower_call(zk, op, a, b=None):
    out = zk.pairing_tower_op(op, F.ints_to_limbs(a), None if b is None else F.ints_to_limbs(b))
    return F.limbs_to_ints(out)


def g1_limbs(p):
    return F.fq_to_mont([0, 0] if p is None else [p[0], p[1]]).reshape(-1)


def g2_limbs(p):
    return F.fq_to_mont([0, 0, 0, 0] if p is None else [p[0][0], p[0][1], p[1][0], p[1][1]]).reshape(-1)
