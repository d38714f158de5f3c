"""The directed cases of the device EdDSA signer (EdDSASigner, zk_eddsa_sign_batch, zk_eddsa_sign_probe).  Pure Python: the expected signatures
come from jubjub_cases.sign -- the restatement that reproduces every pinned value of the reference -- and the expected digests and remainders from
hashlib.sha512 and Python's %.  At import one expected signature of every (scheme, message length) is put through jubjub_cases.verify."""
import hashlib
import random

import jubjub_cases as JC

L, E, Q = JC.L, JC.E, JC.Q
SCHEMES = ("mimc", "pure", "hash")

# SHA-512 pads at total lengths of 111 | 112 and 127 | 128 | 129 bytes; the signer hashes 32 key bytes and the bytes of M: 32 per "mimc" element,
# the message itself for "pure", always 64 for "hash"
LENGTHS = {"pure": [1, 79, 80, 95, 96, 97, 224], "mimc": [1, 3, 4], "hash": [1, 32]}
TOTALS = {"pure": [33, 111, 112, 127, 128, 129, 256], "mimc": [64, 128, 160], "hash": [96, 96]}
B2 = JC.from_hash(b"eddsa_base")                                       # the B of the reference's own test_signverify

KEY_MAX_DIGITS = (5 << 248) | ((1 << 248) - 1)                         # every 4-bit digit below L's top digit (a 6) is 15
KEY_ZERO_DIGITS = int("05" * 32, 16)                                   # a zero digit in every other window
assert (L >> 248) == 6 and KEY_MAX_DIGITS < L and all((KEY_MAX_DIGITS >> (4 * j)) & 15 == 15 for j in range(62))
assert 0 < KEY_ZERO_DIGITS < L and all((KEY_ZERO_DIGITS >> (4 * j)) & 15 == (5 if j % 2 == 0 else 0) for j in range(64))
DIRECTED_KEYS = [1, 2, L - 1, KEY_MAX_DIGITS, KEY_ZERO_DIGITS]
BAD_KEYS = [0, L, L + 1, (1 << 256) - 1]


def keys(n_random=3, seed=71):
    rng = random.Random(seed)
    return DIRECTED_KEYS + [rng.randrange(1, L) for _ in range(n_random)]


_WANT = {}


def frozen(scheme, msg):
    return tuple(msg) if scheme == "mimc" else bytes(msg)


def expected(scheme, key, msg, B=JC.GENERATOR):
    """(A, (R, s)) of jubjub_cases.sign, computed once per (scheme, key, message, base point)"""
    k = (scheme, key, frozen(scheme, msg), B)
    if k not in _WANT:
        A, sig, _ = JC.sign(scheme, msg, key, B)
        _WANT[k] = (A, sig)
    return _WANT[k]


def items(scheme, length, key_list, seed):
    """[(key, msg)]: one seeded message of `length` per key"""
    rng = random.Random(seed * 4099 + length)
    return [(k, JC.make_msg(scheme, length, rng)) for k in key_list]


def length_items(scheme, length):
    """three seeded keys and messages at one message length"""
    rng = random.Random(1000 + length)
    return items(scheme, length, [rng.randrange(1, L) for _ in range(3)], 3)


def key_items(scheme):
    """every directed key and three seeded ones, msg_len 3"""
    return items(scheme, 3, keys(), 5)


for _scheme in SCHEMES:
    assert len(LENGTHS[_scheme]) == len(TOTALS[_scheme])
    for _length, _total in zip(LENGTHS[_scheme], TOTALS[_scheme]):
        _key, _msg = length_items(_scheme, _length)[0]
        assert 32 + len(JC.msg_bytes(_scheme, _msg)) == _total, (_scheme, _length)
        _A, _sig = expected(_scheme, _key, _msg)
        assert JC.verify(_scheme, _A, _sig, _msg), (_scheme, _length)
assert {111, 112, 127, 128, 129} <= set(TOTALS["pure"]) and 128 in TOTALS["mimc"]

# ---------------------------------------------------------------- the probes
SHA_LENGTHS = [0, 1, 111, 112, 127, 128, 129, 239, 240, 255, 256, 257, 1000]


def sha_rows():
    """[(length, [rows of that length])]: two seeded rows and one of all 0xFF per length"""
    rng = random.Random(81)
    return [(n, [bytes(rng.randrange(256) for _ in range(n)) for _ in range(2)] + [b"\xff" * n]) for n in SHA_LENGTHS]


def sha_want(row):
    return hashlib.sha512(row).digest()


def mod_l_cases():
    top = ((1 << 512) - 1) // L * L
    vals = [0, 1, L - 1, L, L + 1, (1 << 256) - 1, 1 << 256, (1 << 512) - 1, top, top - 1, top + 1]
    vals += [L << k for k in (1, 64, 200, 260)]
    vals += [0xFFFFFFFFFFFFFFFF << (64 * i) for i in range(8)]         # all-ones in exactly one limb
    rng = random.Random(82)
    vals += [rng.randrange(1 << 512) for _ in range(200)]
    assert all(0 <= v < 1 << 512 for v in vals) and top + 1 < 1 << 512 and (top + L) >> 512
    return vals


def mod_e_cases():
    """(a, b, c) with a + b c below 2^512"""
    top = (1 << 256) - 1
    cases = [(0, 0, 0), (L - 1, L - 1, Q - 1), (top, top, top)]
    rng = random.Random(83)
    for _ in range(6):                                                 # a + b c = m E - 1, m E, m E + 1
        b, c = rng.randrange(1 << 256), rng.randrange(1 << 256)
        m = b * c // E + 1
        for d in (-1, 0, 1):
            a = m * E + d - b * c
            assert 0 <= a < 1 << 256 and (a + b * c) % E == d % E
            cases.append((a, b, c))
    cases += [(rng.randrange(1 << 256), rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(200)]
    assert all(a + b * c < 1 << 512 for a, b, c in cases)
    return cases
