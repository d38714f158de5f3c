"""What the Baby JubJub tests assert on both builds, shared by test_jubjub_emul.py and test_jubjub_gpu.py: every check takes the binding
(ethsnarks_amd.jubjub with the emulation or the device library loaded) and compares with the restatement of jubjub_cases.py.  Exact comparisons."""
import random

import jubjub_cases as JC

SCHEMES = ("mimc", "pure", "hash")


def pt(v):
    return (int(v[0]), int(v[1]))


def check_constants(J):
    assert (J.JUBJUB_Q, J.JUBJUB_E, J.JUBJUB_L, J.JUBJUB_A, J.JUBJUB_D) == (JC.Q, JC.E, JC.L, JC.A, JC.D)
    assert J.generator() == JC.GENERATOR and J.IDENTITY == JC.IDENTITY


def check_kats(J):
    """every pinned value of tests/golden/jubjub_kats.json through the library"""
    K = JC.KATS
    a = pt(K["point_a"])
    assert J.point_double([a]) == [pt(K["point_a_double"])] == J.point_add([a], [a])
    assert J.scalar_mul([a], [2]) == [pt(K["point_a_double"])]
    assert J.scalar_mul([a], [int(K["mult_known"]["scalar"])]) == [pt(K["mult_known"]["result"])]
    assert J.hash_to_point(b"test") == pt(K["from_hash_test"])
    for x, y in K["from_y"]:                                           # the sign rule of from_y, as the restatement applies it in from_hash
        assert JC.from_y(int(y)) == (int(x), int(y))
    low = [pt(p) for p in K["low_order"]]
    assert J.scalar_mul(low, [8] * 8) == [JC.IDENTITY] * 8
    assert J.scalar_mul(low[1:], [JC.L] * 7) == low[1:]               # test_loworder: L p == p
    with J.PedersenHasher("test", 256) as h:
        for c in K["pedersen_scalars"]:
            assert h.hash_scalars([[int(c["scalar"])]]) == [pt(c["result"])]
        for c in K["pedersen_bytes"]:
            assert h.hash_bytes([c["data"].encode()]) == [pt(c["result"])]
    for c in K["pedersen_bits"]:
        with J.PedersenHasher(c["name"], len(c["bits"])) as h:
            assert h.hash_bits([c["bits"]]) == [pt(c["result"])]
    e = K["eddsa"]["mimc"]
    with J.EdDSAVerifier("mimc", msg_len=3) as v:
        assert v.verify([pt(e["A"])], [(pt(e["R"]), int(e["s"]))], [[int(m) for m in e["msg"]]]) == [True]
    for scheme, other in (("hash", "pure"), ("pure", "hash")):         # the reference's own cross checks
        e = K["eddsa"][scheme]
        args = ([pt(e["A"])], [(pt(e["R"]), int(e["s"]))], [e["msg"].encode()])
        with J.EdDSAVerifier(scheme, msg_len=len(e["msg"])) as v:
            assert v.verify(*args) == [True]
        with J.EdDSAVerifier(other, msg_len=len(e["msg"])) as v:
            assert v.verify(*args) == [False]


def check_hash_to_point(J):
    for data in (b"", b"test", b"eddsa_base", bytes(range(70))):
        assert J.hash_to_point(data) == JC.from_hash(data), data
    for name, i in ((b"test", 0), ("EdDSA_Verify.RAM", 4), (b"", 0xFFFF), (b"x" * 28, 1)):
        assert J.pedersen_basepoint(name, i) == JC.basepoint(name, i), (name, i)


def spread(items, n):
    """n items: the directed ones first and again at the end (the first and the last lanes), cycled in between"""
    out = [items[i % len(items)] for i in range(n)]
    tail = items[-min(len(items), n):]
    out[n - len(tail):] = tail
    return out


def check_point_ops(J, n_random, sizes=None):
    pairs = JC.point_pairs()
    rnd = JC.random_points(2 * n_random, 21)
    pairs += list(zip(rnd[:n_random], rnd[n_random:]))
    want = {}
    for p, q in pairs:
        want[(p, q)] = JC.add(p, q)
    for n in sizes or [len(pairs)]:
        use = spread(pairs, n)
        got = J.point_add([p for p, _ in use], [q for _, q in use])
        assert got == [want[k] for k in use], n
    singles = JC.POINTS + rnd
    assert J.point_double(singles) == [JC.double(p) for p in singles]
    assert J.point_neg(singles) == [JC.neg(p) for p in singles]
    assert J.point_neg([JC.IDENTITY]) == [JC.IDENTITY]
    for p, q in pairs[:12]:                                            # the projective restatement against the reference's affine formula
        assert JC.add(p, q) == JC.affine_add_reference(p, q)


_MUL_WANT = {}


def check_scalar_mul(J, n_random, sizes=None):
    cases = JC.scalar_cases()
    rng = random.Random(31)
    cases += [(p, rng.randrange(1 << 256)) for p in JC.random_points(n_random, 32)]
    for c in cases:
        if c not in _MUL_WANT:
            _MUL_WANT[c] = JC.mul(*c)
    for n in sizes or [len(cases)]:
        use = spread(cases, n)
        got = J.scalar_mul([p for p, _ in use], [k for _, k in use])
        bad = [(i, use[i][1]) for i in range(n) if got[i] != _MUL_WANT[use[i]]]
        assert not bad, "n = %d: %d wrong, the first: item %d, scalar 0x%x" % (n, len(bad), bad[0][0], bad[0][1])


_PED_WANT = {}


def check_pedersen(J, sizes=None):
    rows = JC.window_rows()
    for r in rows:
        if tuple(r) not in _PED_WANT:
            _PED_WANT[tuple(r)] = JC.pedersen_windows(b"test", r)
    with J.PedersenHasher(b"test", 3 * 125) as h:
        assert h.max_windows == 125
        for n in sizes or [len(rows)]:
            use = spread(rows, n)                                      # ragged counts in every wave
            assert h.hash_windows(use) == [_PED_WANT[tuple(r)] for r in use], n
        full = [r for r in rows if len(r) == 125]
        assert h.hash_windows(full) == [_PED_WANT[tuple(r)] for r in full]   # counts == stride for every row
        cancel = [r for r in rows if len(r) == 62][-2:]
        a, b = h.hash_windows(cancel)
        assert J.point_add([a], [b]) == [JC.IDENTITY]
        bits = [[(i * 7 + j) % 3 % 2 for j in range(c)] for i, c in enumerate((1, 2, 3, 4, 374, 375))]
        assert h.hash_bits(bits) == [JC.pedersen_bits(b"test", b) for b in bits]
        assert h.hash_scalars([[0], [5, 0, 9], [JC.Q - 1]]) == [JC.IDENTITY, JC.pedersen_scalars(b"test", 5, 0, 9), JC.pedersen_scalars(b"test", JC.Q - 1)]


def check_tables(J):
    """the hasher's table against the restatement for two segments"""
    with J.PedersenHasher(b"test", 3 * 124) as h:
        got = h.table(0, 124)
    for j in range(124):
        assert got[j] == [JC.affine(p) for p in JC.table_row(b"test", j)], j
    assert got[62][0] == JC.basepoint(b"test", 1) and got[1][0] == JC.mul(JC.basepoint(b"test", 0), 16)


_SIG_CASES = {}


def sig_cases(scheme, length, B=JC.GENERATOR):
    key = (scheme, length, B)
    if key not in _SIG_CASES:
        _SIG_CASES[key] = JC.signature_cases(scheme, length, B)
    return _SIG_CASES[key]


def run_cases(J, scheme, length, cases, B=None, n=None):
    use = spread(cases, n) if n else cases
    with J.EdDSAVerifier(scheme, B=B, msg_len=length) as v:
        got = v.verify([c[1] for c in use], [c[2] for c in use], [c[3] for c in use])
    bad = [(i, use[i][0]) for i in range(len(use)) if got[i] != use[i][4]]
    assert not bad, "%s, msg_len %d: wrong verdicts for %s" % (scheme, length, bad[:5])


def check_signatures(J, scheme, sizes=None):
    """the directed signatures at the first message length, at every n; the other lengths and the custom base once"""
    lengths = JC.other_lengths(scheme)
    for n in sizes or [None]:
        run_cases(J, scheme, 3, sig_cases(scheme, 3), n=n)
    for length in lengths:
        if length != 3:
            run_cases(J, scheme, length, sig_cases(scheme, length)[:6])
    B = JC.from_hash(b"eddsa_base")
    run_cases(J, scheme, 4, sig_cases(scheme, 4, B)[:4], B=B)
    with J.EdDSAVerifier(scheme, msg_len=4) as v:                      # signed over the other base: the generator's verifier refuses it
        c = sig_cases(scheme, 4, B)[0]
        assert v.verify([c[1]], [c[2]], [c[3]]) == [False]


def check_cross_scheme(J):
    """a hash-scheme signature offered to the pure verifier and the reverse"""
    for scheme, other in (("hash", "pure"), ("pure", "hash")):
        c = sig_cases(scheme, 3)[0]
        with J.EdDSAVerifier(other, msg_len=3) as v:
            assert v.verify([c[1]], [c[2]], [c[3]]) == [False]
