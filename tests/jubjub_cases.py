"""A Python-integer restatement of the reference's Baby JubJub code (ethsnarks/jubjub.py, pedersen.py, eddsa.py, mimc/permutation.py) and the
directed cases of the Baby JubJub tests.  Projective arithmetic with one final inversion; plain ints, no field class.  Every case list asserts from
this restatement alone that it holds what it claims.  The pinned values of tests/golden/jubjub_kats.json tie the restatement to the reference."""
import hashlib
import json
import os
import random

from ethsnarks_amd import gadgets as G

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
E = 21888242871839275222246405745257275088614511777268538073601725287587578984328
L = E // 8
A, D = 168700, 168696
IDENTITY = (0, 1)
GENERATOR = (16540640123574156134436876038791482806971768689494387082833631921987005038935,
             20819045374670962167435360035096875258406992893633759881276124905556507972311)
SEG = 62

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jubjub_kats.json")) as _f:
    KATS = json.load(_f)


def _pt(v):
    return (int(v[0]), int(v[1]))


POINT_A = _pt(KATS["point_a"])
LOW_ORDER = [_pt(p) for p in KATS["low_order"]]


# ---------------------------------------------------------------- curve (EtecPoint.add / double, without the identity shortcut: the formulas are complete)
def on_curve(p):
    x, y = p
    return (A * x * x + y * y - 1 - D * x * x * y * y) % Q == 0


def ext(p):
    return (p[0], p[1], p[0] * p[1] % Q, 1)


def eadd(p, q):
    x1, y1, t1, z1 = p
    x2, y2, t2, z2 = q
    a, b, c, d = x1 * x2 % Q, y1 * y2 % Q, D * t1 * t2 % Q, z1 * z2 % Q
    e = ((x1 + y1) * (x2 + y2) - a - b) % Q
    f, g, h = (d - c) % Q, (d + c) % Q, (b - A * a) % Q
    return (e * f % Q, g * h % Q, e * h % Q, f * g % Q)


def edbl(p):
    x, y, _, z = p
    a, b, c = x * x % Q, y * y % Q, 2 * z * z % Q
    d = A * a % Q
    e = ((x + y) * (x + y) - a - b) % Q
    g = (d + b) % Q
    f, h = (g - c) % Q, (d - b) % Q
    return (e * f % Q, g * h % Q, e * h % Q, f * g % Q)


def affine(p):
    zi = pow(p[3], Q - 2, Q)
    assert p[3] % Q != 0
    return (p[0] * zi % Q, p[1] * zi % Q)


def eneg(p):
    return (-p[0] % Q, p[1], -p[2] % Q, p[3])


def emul(p, k):
    """AbstractCurveOps.mult: double and add from the low bit; any k >= 0"""
    acc = ext(IDENTITY)
    while k:
        if k & 1:
            acc = eadd(acc, p)
        p = edbl(p)
        k >>= 1
    return acc


def add(p, q):
    return affine(eadd(ext(p), ext(q)))


def double(p):
    return affine(edbl(ext(p)))


def neg(p):
    return (-p[0] % Q, p[1])


def mul(p, k):
    return affine(emul(ext(p), int(k)))


def affine_add_reference(p, q):
    """Point.add of the reference: the affine formula with two divisions (what its verify() runs)"""
    (u1, v1), (u2, v2) = p, q
    w = D * u1 * u2 * v1 * v2
    return ((u1 * v2 + v1 * u2) * pow(1 + w, Q - 2, Q) % Q, (v1 * v2 - A * u1 * u2) * pow(1 - w, Q - 2, Q) % Q)


# ---------------------------------------------------------------- hash to point
def sqrt_mod(a):
    """Tonelli-Shanks; None for a non-residue"""
    a %= Q
    if a == 0:
        return 0
    if pow(a, (Q - 1) // 2, Q) != 1:
        return None
    s, q = 0, Q - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    z = 2
    while pow(z, (Q - 1) // 2, Q) != Q - 1:
        z += 1
    m, c, t, r = s, pow(z, q, Q), pow(a, q, Q), pow(a, (q + 1) // 2, Q)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u, i = u * u % Q, i + 1
        b = pow(c, 1 << (m - i - 1), Q)
        m, c, t, r = i, b * b % Q, t * b * b % Q, r * b % Q
    return r


def from_y(y):
    """Point.from_y without a sign: x^2 = (y^2 - 1) / (d y^2 - a), x the root with x > r - x; None when there is none"""
    ysq = y * y % Q
    x = sqrt_mod((ysq - 1) * pow(D * ysq - A, Q - 2, Q))
    if x is None:
        return None
    if x < (-x) % Q:
        x = (-x) % Q
    return (x, y)


def from_hash(data):
    y = int.from_bytes(hashlib.sha256(data).digest(), "big") % Q
    while True:
        p = from_y(y)
        if p is not None:
            return mul(p, 8)
        y = (y + 1) % Q


# ---------------------------------------------------------------- Pedersen
_BASE = {}


def basepoint(name, i):
    name = name.encode("ascii") if isinstance(name, str) else name
    assert 0 <= i <= 0xFFFF and len(name) <= 28
    if (name, i) not in _BASE:
        _BASE[(name, i)] = from_hash(b"%-28s%04X" % (name, i))
    return _BASE[(name, i)]


_TABLE = {}


def table_row(name, j):
    """[(1 .. 4) 16^(j % 62) B_(j / 62)] as extended points"""
    name = name.encode("ascii") if isinstance(name, str) else name
    if (name, j) not in _TABLE:
        cur = ext(basepoint(name, j // SEG)) if j % SEG == 0 else edbl(edbl(table_row(name, j - 1)[3]))
        m2 = edbl(cur)
        _TABLE[(name, j)] = [cur, m2, eadd(m2, cur), edbl(m2)]
    return _TABLE[(name, j)]


def pedersen_windows(name, windows):
    for j in range(len(windows)):                                      # (fills the table without deep recursion)
        table_row(name, j)
    acc = ext(IDENTITY)
    for j, w in enumerate(windows):
        seg = table_row(name, j)[w & 3]
        acc = eadd(acc, eneg(seg) if w > 3 else seg)
    return affine(acc)


def bits_to_windows(bits):
    bits = [int(b) for b in bits]
    return [sum(b << k for k, b in enumerate(bits[i:i + 3])) for i in range(0, len(bits), 3)]


def bytes_to_bits(data):
    return [int(c) for byte in data for c in bin(byte)[2:].rjust(8, "0")]


def field_bits(v):
    return [(v >> i) & 1 for i in range(254)]


def scalars_to_windows(scalars):
    return [(s >> i) & 7 for s in scalars for i in range(0, s.bit_length(), 3)]


def pedersen_bits(name, bits):
    return pedersen_windows(name, bits_to_windows(bits))


def pedersen_bytes(name, data):
    return pedersen_bits(name, bytes_to_bits(data))


def pedersen_scalars(name, *scalars):
    return pedersen_windows(name, scalars_to_windows(scalars))


# ---------------------------------------------------------------- EdDSA
RAM, MSG = b"EdDSA_Verify.RAM", b"EdDSA_Verify.M"
_RAM_C = None


def mimc_hash_ram(xs):
    global _RAM_C
    if _RAM_C is None:
        _RAM_C = G.mimc_constants(seed=RAM)
    k = 0
    for x in xs:
        v = x
        for c in _RAM_C:
            v = pow((v + k + c) % Q, 7, Q)
        k = (k + x + v + k) % Q
    return k


def hash_public(scheme, R, Apt, msg):
    if scheme == "mimc":
        return mimc_hash_ram([R[0], R[1], Apt[0], Apt[1]] + [int(m) for m in msg])
    tail = field_bits(pedersen_bytes(MSG, msg)[0]) if scheme == "hash" else bytes_to_bits(msg)
    return pedersen_bits(RAM, field_bits(R[0]) + field_bits(Apt[0]) + tail)[0]


def msg_bytes(scheme, msg):
    if scheme == "mimc":
        return b"".join(int(m).to_bytes(32, "little") for m in msg)
    return pedersen_bytes(MSG, msg)[0].to_bytes(32, "little") + pedersen_bytes(MSG, msg)[1].to_bytes(32, "little") if scheme == "hash" else bytes(msg)


def sign(scheme, msg, key, B=GENERATOR):
    """_SignatureScheme.sign: r = sha512(k || M) mod L, R = r B, S = (r + k t) mod E"""
    assert 0 < key < L
    Apt = mul(B, key)
    r = int.from_bytes(hashlib.sha512(key.to_bytes(32, "little") + msg_bytes(scheme, msg)).digest(), "little") % L
    R = mul(B, r)
    t = hash_public(scheme, R, Apt, msg)
    return Apt, (R, (r + key * t) % E), msg


def verify(scheme, Apt, sig, msg, B=GENERATOR):
    """the library's verdict: False for A or R off the curve, else the reference's S B == R + t A"""
    R, s = sig
    if not on_curve(Apt) or not on_curve(R):
        return False
    t = hash_public(scheme, R, Apt, msg)
    return mul(B, s) == affine(eadd(ext(R), emul(ext(Apt), t)))


# ---------------------------------------------------------------- directed cases
def max_digit_scalar():
    return (1 << 256) - 1                                              # every 4-bit window digit is 15, every bit is set


SCALARS = [0, 1, 2, 8, L - 1, L, L + 1, E - 1, E, E + 1, 1 << 251, Q - 1, (1 << 256) - 1, max_digit_scalar(), 0x8888888888888888888888888888888888888888888888888888888888888888,
           0x1111111111111111111111111111111111111111111111111111111111111111]
assert all(0 <= k < 1 << 256 for k in SCALARS) and {0, L, E, E + 1, (1 << 256) - 1} <= set(SCALARS) and max(SCALARS) >= E
assert all((max_digit_scalar() >> (4 * j)) & 15 == 15 for j in range(64))

assert len(LOW_ORDER) == 8 and LOW_ORDER[0] == IDENTITY and all(on_curve(p) and mul(p, 8) == IDENTITY for p in LOW_ORDER)
assert sum(p[1] == 0 for p in LOW_ORDER) == 2 and len(set(LOW_ORDER)) == 8
assert on_curve(GENERATOR) and on_curve(POINT_A) and mul(GENERATOR, L) == IDENTITY

POINTS = LOW_ORDER + [GENERATOR, POINT_A]


def point_pairs():
    """(p, q) for the addition: every directed point with the generator and with itself, P with -P, the identity on either side, low order
    with low order"""
    pairs = [(p, GENERATOR) for p in POINTS] + [(p, p) for p in POINTS] + [(p, neg(p)) for p in POINTS]
    pairs += [(IDENTITY, p) for p in POINTS] + [(p, IDENTITY) for p in POINTS]
    pairs += [(p, q) for p in LOW_ORDER for q in LOW_ORDER]
    assert all(add(p, neg(p)) == IDENTITY for p in POINTS)
    assert (POINT_A, POINT_A) in pairs and (GENERATOR, neg(GENERATOR)) in pairs and (IDENTITY, IDENTITY) in pairs
    return pairs


def random_points(n, seed):
    rng = random.Random(seed)
    return [mul(GENERATOR, rng.randrange(1, L)) for _ in range(n)]


def scalar_cases():
    """(point, scalar): every directed scalar on the generator and on point a, a few on every low-order point"""
    cases = [(p, k) for p in (GENERATOR, POINT_A) for k in SCALARS]
    cases += [(p, k) for p in LOW_ORDER for k in (0, 1, 7, 8, L, (1 << 256) - 1)]
    return cases


WINDOW_COUNTS = [1, 2, 61, 62, 63, 124, 125]


def window_rows():
    """rows for one hasher of capacity 125: the segment boundaries, constant rows, rows that cancel, ragged counts"""
    rng = random.Random(11)
    rows = [[rng.randrange(8) for _ in range(c)] for c in WINDOW_COUNTS]
    rows += [[w] * c for w in (0, 3, 4, 7) for c in (1, 62, 125)]
    cancel = [rng.randrange(8) for _ in range(62)]
    rows += [cancel, [w ^ 4 for w in cancel]]                          # the second hashes to the negative of the first
    rows += [[rng.randrange(8) for _ in range(rng.randrange(1, 126))] for _ in range(12)]
    assert {len(r) for r in rows} >= set(WINDOW_COUNTS)
    a, b = pedersen_windows(b"test", cancel), pedersen_windows(b"test", [w ^ 4 for w in cancel])
    assert b == neg(a) and add(a, b) == IDENTITY
    return rows


def other_lengths(scheme):
    return [1, 3] if scheme == "mimc" else [1, 3, 4, 32]


def make_msg(scheme, length, rng):
    if scheme == "mimc":
        return [rng.randrange(Q) for _ in range(length)]
    return bytes(rng.randrange(256) for _ in range(length))


def flip_first(scheme, msg):
    return [(msg[0] + 1) % Q] + list(msg[1:]) if scheme == "mimc" else bytes([msg[0] ^ 0x80]) + msg[1:]


def flip_last(scheme, msg):
    return list(msg[:-1]) + [(msg[-1] + 1) % Q] if scheme == "mimc" else msg[:-1] + bytes([msg[-1] ^ 1])


OFF_CURVE = (1, 1)
assert not on_curve(OFF_CURVE)


def signature_cases(scheme, length, B=GENERATOR, seed=5):
    """[(label, A, (R, s), msg, verdict)]: the verdict comes from verify() above and is asserted against what the label claims"""
    rng = random.Random(seed * 1000 + length)
    msg = make_msg(scheme, length, rng)
    while True:                                                        # (a key whose s leaves room for s + L below r: 7 of 8 do)
        Apt, (R, s), _ = sign(scheme, msg, rng.randrange(1, L), B)
        if s + L < Q:
            break
    other = mul(B, rng.randrange(1, L))
    low = LOW_ORDER[3]
    cases = [("valid", Apt, (R, s), msg, True),
             ("s + 1", Apt, (R, (s + 1) % Q), msg, False),
             ("R replaced", Apt, (other, s), msg, False),
             ("A replaced", other, (R, s), msg, False),
             ("first bit of the message", Apt, (R, s), flip_first(scheme, msg), False),
             ("last bit of the message", Apt, (R, s), flip_last(scheme, msg), False),
             ("A = identity, R = s B", IDENTITY, (mul(B, s), s), msg, True),
             ("A = R = identity, s = 0", IDENTITY, (IDENTITY, 0), msg, True),
             ("low-order A", low, (R, s), msg, None),
             ("off-curve A", OFF_CURVE, (R, s), msg, False),
             ("off-curve R", Apt, (OFF_CURVE, s), msg, False),
             ("s + L", Apt, (R, s + L), msg, True)]
    out = []
    for label, a, sig, m, want in cases:
        got = verify(scheme, a, sig, m, B)
        assert want is None or got == want, (scheme, label)
        out.append((label, a, sig, m, got))
    return out


def batch(scheme, length, n, B=GENERATOR, seed=9):
    """n signatures, valid and invalid interleaved: (A, sigs, msgs, verdicts)"""
    rng = random.Random(seed)
    base = [sign(scheme, make_msg(scheme, length, rng), rng.randrange(1, L), B) for _ in range(8)]
    A_, sigs, msgs, want = [], [], [], []
    for i in range(n):
        a, (R, s), m = base[i % 8]
        kind = (i * 7 + i // 8) % 4
        if kind == 1:
            s = (s + 1 + i) % Q
        elif kind == 2:
            m = flip_last(scheme, m)
        elif kind == 3 and i % 3 == 0:
            R = base[(i + 1) % 8][1][0]
        A_.append(a); sigs.append((R, s)); msgs.append(m)
    memo = {}
    for a, sig, m in zip(A_, sigs, msgs):
        key = (a, sig, bytes(m) if scheme != "mimc" else tuple(m))
        if key not in memo:
            memo[key] = verify(scheme, a, sig, m, B)
        want.append(memo[key])
    assert any(want) and not all(want)
    assert all(len(set(want[w:w + 64])) == 2 for w in range(0, n - 1, 64) if len(want[w:w + 64]) > 1)   # no uniform wave
    return A_, sigs, msgs, want
