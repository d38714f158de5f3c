"""The per-key kernels of the four-transform prover (csrc/hlagrange.hpp) on their own, against big-integer sums: the G1 group DFT
(zk_hl_probe_dft) at m = 2^3 .. 2^10 and the column sums K_v (zk_hl_probe_columns).

Every input point is a known multiple s_i G of the generator, so the expected output j is (sum_i coefficient_ij s_i mod r) G: the direct
sum is taken over the integers and one fixed-base multiplication per output (big-int Jacobian arithmetic, below) gives the point.  The
inputs are chosen for the exceptional cases of the group law: all inputs equal (P + P in every first-stage butterfly, P - P = O into the
twiddle multiplication), points at infinity, and P, -P pairs half a domain apart (O out of the butterfly's sum)."""
import random

import pytest
import pyref as P
from ethsnarks_amd import r1cs as R

pytestmark = pytest.mark.gpu
FR, FQ = P.R, P.Q


# ---- big-int G1 in Jacobian coordinates (y^2 = x^3 + 3): no inversion per operation
def _jdbl(p):
    if p is None:
        return None
    X, Y, Z = p
    if Y == 0:
        return None
    A, B = X * X % FQ, Y * Y % FQ
    Cc = B * B % FQ
    D = 2 * ((X + B) ** 2 - A - Cc) % FQ
    E = 3 * A % FQ
    X3 = (E * E - 2 * D) % FQ
    return X3, (E * (D - X3) - 8 * Cc) % FQ, 2 * Y * Z % FQ


def _jadd(p, q):
    if p is None:
        return q
    if q is None:
        return p
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    Z1Z1, Z2Z2 = Z1 * Z1 % FQ, Z2 * Z2 % FQ
    U1, U2 = X1 * Z2Z2 % FQ, X2 * Z1Z1 % FQ
    S1, S2 = Y1 * Z2 * Z2Z2 % FQ, Y2 * Z1 * Z1Z1 % FQ
    if U1 == U2:
        return _jdbl(p) if S1 == S2 else None
    H, Rr = (U2 - U1) % FQ, (S2 - S1) % FQ
    HH = H * H % FQ
    HHH, V = H * HH % FQ, U1 * HH % FQ
    X3 = (Rr * Rr - HHH - 2 * V) % FQ
    return X3, (Rr * (V - X3) - S1 * HHH) % FQ, Z1 * Z2 * H % FQ


_TABLE = []                                                          # _TABLE[w][d] = d 16^w G, built once


def _gen_mul(k):
    if not _TABLE:
        base = (P.G1_GEN[0], P.G1_GEN[1], 1)
        for _ in range(64):
            row, acc = [None], None
            for _ in range(15):
                acc = _jadd(acc, base); row.append(acc)
            _TABLE.append(row)
            base = _jadd(acc, base)
    acc, k = None, k % FR
    for w in range(64):
        acc = _jadd(acc, _TABLE[w][(k >> (4 * w)) & 15])
    return acc


def _same(affine, jac):
    if affine is None or jac is None:
        return affine is None and jac is None
    X, Y, Z = jac
    zz = Z * Z % FQ
    return affine[0] * zz % FQ == X and affine[1] * zz * Z % FQ == Y


def _affine(jac):
    if jac is None:
        return None
    zi = pow(jac[2], -1, FQ)
    return jac[0] * zi * zi % FQ, jac[1] * zi * zi * zi % FQ


def _inputs(kind, m, rng):
    """discrete logarithms of the m - 1 input points (0: the point at infinity)"""
    n = m - 1
    if kind == "random":
        s = set()
        while len(s) < n:
            s.add(rng.randrange(1, FR))
        return sorted(s, key=lambda v: v * 7919 % FR)                 # distinct, in no particular order
    if kind == "equal":
        return [rng.randrange(1, FR)] * n
    s = [rng.randrange(1, FR) for _ in range(n)]                      # "special": infinities, and P, -P pairs half a domain apart and adjacent
    for i in range(0, n, 5):
        s[i] = 0
    for i in range(1, m // 2 - 1, 3):
        s[i + m // 2] = FR - s[i]
    if n > 3:
        s[3] = FR - s[2]
    return s


@pytest.mark.parametrize("logm", range(3, 11))
def test_group_dft_against_direct_sum(hip, logm):
    m = 1 << logm
    rng = random.Random(logm)
    w_inv, g_inv = pow(P.omega(m), -1, FR), pow(P.COSET_G, -1, FR)
    k = pow(m * (pow(P.COSET_G, m, FR) - 1), -1, FR)
    wp = [pow(w_inv, e, FR) for e in range(m)]
    for n_kind, kind in enumerate(("random", "equal", "special")):
        for cs in ((logm + n_kind) & 1,):                              # both scalings at every size over the three inputs, every pairing over the sizes
            s = _inputs(kind, m, rng)
            pts = [_affine(_gen_mul(v)) if v else None for v in s]
            got = hip.hl_probe_dft(pts, logm, cs)
            pre = [v * (pow(g_inv, i, FR) if cs else 1) % FR for i, v in enumerate(s)]
            for j in range(m):
                e = k * sum(pre[i] * wp[i * j % m] for i in range(m - 1)) % FR
                assert _same(got[j], _gen_mul(e) if e else None), (kind, cs, j)


def test_column_sums_against_big_int(hip):
    """K_v on a matrix with empty columns, a column of 300 entries (three chunks of HL_COL_CHUNK = 128) with coefficients 1, -1 and random,
    Lambda with points at infinity and a P, -P pair inside the long column (its running sum passes through O)"""
    m, nC, nIn, V = 512, 300, 2, 10
    rng = random.Random(11)
    lam = [rng.randrange(1, FR) for _ in range(m)]
    for j in range(0, m, 7):
        lam[j] = 0
    lam[1], lam[2] = 5, FR - 5
    rows = []
    for j in range(nC):
        coef = 1 if j < 120 else (FR - 1 if j < 240 else rng.randrange(2, FR - 1))
        row = [(3, coef)]                                             # column 3: every row
        if j % 3 == 0:
            row.append((7 + j % 4, rng.choice([1, FR - 1, rng.randrange(FR)])))
        if j == 17:
            row.append((0, FR - 1))                                   # the constant ONE once, a public input (v = 2) below; columns 1, 4, 5, 6 stay empty
        if j == 18:
            row.append((2, rng.randrange(FR)))
        rows.append(row)
    Cm = R.CSR.from_rows(rows)
    l_log = [rng.randrange(FR) for _ in range(V - nIn)]
    l_log[1] = 0                                                      # L_4 = O and column 4 empty: O out
    got = hip.hl_probe_columns(Cm, nIn, V, [_affine(_gen_mul(v)) if v else None for v in lam], [_affine(_gen_mul(v)) if v else None for v in l_log])
    K = [0] * (V + 1)
    for j, row in enumerate(rows):
        for v, coef in row:
            K[v] = (K[v] + coef * lam[j]) % FR
    for v in range(V + 1):
        e = ((l_log[v - nIn - 1] if v > nIn else 0) - K[v]) % FR
        assert _same(got[v], _gen_mul(e) if e else None), v
    assert got[1] is None and got[4] is None and got[3] is not None
