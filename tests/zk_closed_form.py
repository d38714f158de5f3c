"""Zero-knowledge Groth16 proofs in closed form from the toxic waste (libsnark's r1cs_gg_ppzksnark_prover with the zok generator's key
elements): the sums of pyref.proof_from_trapdoor, extended by the blinding scalars r, s

    A = (alpha + SA + r delta) G1,   B = (beta + SB + s delta) G2,
    C = (c0 + s (alpha + SA) + r (beta + SB) + r s delta) G1,

where c0 delta G1 ... is the no-ZK C.  Slow big-int code (m <= 2^10); shared by the CPU and GPU tests."""
import pyref
from pyref import R


def trapdoor_sums(r1cs, w, t, alpha, beta, gamma, delta):
    """(SA, SB, c0): SA = sum_i w_i A_i(t), SB = sum_i w_i B_i(t), c0 = the no-ZK C's scalar (pyref.proof_from_trapdoor's sums)"""
    nC, nIn, V, A, B, C = r1cs
    m = pyref.domain_size(nC, nIn)
    om = pyref.omega(m)
    Zt = (pow(t, m, R) - 1) % R
    wj, den, pre, acc = 1, [], [], 1
    for j in range(m):
        d = m * (t - wj) % R
        den.append(d); pre.append(acc); acc = acc * d % R
        wj = wj * om % R
    inv = pow(acc, -1, R)
    u = [0] * m
    wpow = pow(om, m - 1, R); omi = pow(om, -1, R)
    for j in range(m - 1, -1, -1):
        u[j] = wpow * Zt % R * (inv * pre[j] % R) % R
        inv = inv * den[j] % R
        wpow = wpow * omi % R

    def evaluate(rows):
        tot = pub = 0
        for j, row in enumerate(rows):
            for i, c in row:
                v = c * w[i] % R * u[j]
                tot += v
                if i <= nIn:
                    pub += v
        return tot % R, pub % R
    SA, pA = evaluate(A); SB, pB = evaluate(B); SC, pC = evaluate(C)
    for i in range(nIn + 1):
        v = u[nC + i] * w[i] % R
        SA = (SA + v) % R; pA = (pA + v) % R
    priv = (beta * (SA - pA) + alpha * (SB - pB) + (SC - pC)) % R
    c0 = (priv + SA * SB - SC) * pow(delta, -1, R) % R
    return SA, SB, c0


def zk_scalars(sums, toxic, r, s):
    """the discrete logs (a, b, c) of the zero-knowledge proof's A (G1), B (G2), C (G1)"""
    SA, SB, c0 = sums
    _, alpha, beta, _, delta = toxic
    a, b = (alpha + SA) % R, (beta + SB) % R
    return (a + r * delta) % R, (b + s * delta) % R, (c0 + s * a + r * b + r * s * delta) % R


def zk_proof_json(r1cs, w, toxic, r, s, sums=None):
    sums = sums or trapdoor_sums(r1cs, w, *toxic)
    a, b, c = zk_scalars(sums, toxic, r, s)
    nIn = r1cs[1]
    return pyref.proof_to_json(pyref.g1_mul(pyref.G1_GEN, a), pyref.g2_mul(pyref.G2_GEN, b), pyref.g1_mul(pyref.G1_GEN, c), w[1:1 + nIn])


def r_for_infinite_A(sums, toxic):
    """r with alpha + SA + r delta = 0: A is the point at infinity"""
    SA = sums[0]
    return (-(toxic[1] + SA)) * pow(toxic[4], -1, R) % R


def s_for_infinite_B(sums, toxic):
    """s with beta + SB + s delta = 0: B and B1 are the point at infinity"""
    SB = sums[1]
    return (-(toxic[2] + SB)) * pow(toxic[4], -1, R) % R
