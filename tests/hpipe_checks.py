"""Checks of the H pipeline through its two probes, on the cases of hpipe_cases.py.  They run unchanged on the CPU stand-in
(test_hpipe_emul.py) and on the device (test_hpipe_gpu.py); `zk` is the ethsnarks_amd.prover module with a library loaded, `oracle` the CPU
oracle's binding.  Everything is integer arithmetic and every comparison is bit-exact: there is no tolerance anywhere.

  (a) check_ntt_case        zk_ntt_probe against Python integers (pyref.ntt / intt / omega, the scaling tables written out as pow) for
                            logm <= 13; above that against the oracle's transform composed with elementwise products (orc_fr_mul) by
                            geometric tables that Python builds.  The gaps behind the vectors must hold the sentinel.
  (b) check_ntt_refusals    the transform probe's argument checks; a refused call writes nothing
  (c) check_h_stages        zk_ctx_probe_h: every buffer of every proof against a reference built from Python dot products and pyref's
                            transforms, h and h[m-1] against the oracle's witness map as a second opinion
  (d) check_degree_refusal  a batch whose MIDDLE witness is wrong is refused with ZK_ERR_DEGREE; the context then proves the good batch
  (e) check_h_refusals      the H probe's argument checks

What a word means (include/zkhip.h, read from the kernels): the transform is linear on the stored words, a product with a table entry
T (stored as T R) maps a word x to x T, and a product of two stored words x, y gives x y / R.  So the transform reference works on the words
themselves, and the H reference converts explicitly: mont(v) = v R for a Montgomery buffer, v itself for a canonical one."""
import ctypes as C
import functools
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import hpipe_cases as cases
import pyref

ZK_ERR_ARG, ZK_ERR_DEGREE = 1, 7
FR, G = F.FR, 5
assert pyref.R == FR and pyref.COSET_G == G
ORACLE_FROM = 14                                  # logm from which the oracle's transform is the reference


def mont(vals):
    return [v * F.MONT_R % FR for v in vals]


def first_difference(got, want, where, unit="index"):
    """got, want: (vectors, n, 4) limbs.  Fails naming the first wrong (vector, index), both values and how many are wrong."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    if bad.size:
        v, i = int(bad[0][0]), int(bad[0][1])
        pytest.fail("%s: vector %d, %s %d is wrong (%d elements are, in vectors %s): got %#x, expected %#x"
                    % (where, v, unit, i, len(bad), sorted({int(b[0]) for b in bad}), F.limbs_to_ints(got[v, i])[0], F.limbs_to_ints(want[v, i])[0]))


# ---------------------------------------------------------------- (a), (b): one ntt_run
def scale_of(name, m):
    """(s, b): the table `name` of NttTables holds s b^i at i"""
    mi, gi = pow(m, -1, FR), pow(G, -1, FR)
    zinv = pow(pow(G, m, FR) - 1, -1, FR)
    return {"none": None, "inv_m": (mi, 1), "icoset": (mi, gi), "inv_then_coset": (mi, G), "inv_m_zinv": (mi * zinv % FR, 1),
            "icoset_zinv": (mi * zinv % FR, gi)}[name]


def geometric(s, b, m):
    out, t = [], s % FR
    for _ in range(m):
        out.append(t); t = t * b % FR
    return out


def post_of(case, v):
    return case.post_alt if case.post_alt != "none" and v >= case.alt_from else case.post


def reference_ints(case, x, x2, sub):
    """(batch, m, 4) limbs of what ntt_run must leave, with Python integers"""
    m = 1 << case.logm
    w = pyref.omega(m)
    if case.inverse:
        w = pow(w, -1, FR)
    pre = geometric(1, G, m) if case.pre == "coset_fwd" else None
    tables = {name: geometric(*scale_of(name, m), m) for name in {post_of(case, v) for v in range(case.batch)} if name != "none"}
    out = []
    for v in range(case.batch):
        a = [t % FR for t in F.limbs_to_ints(x[v, :m])]
        if x2 is not None:
            a = [s * t * F.FR_RINV % FR for s, t in zip(a, F.limbs_to_ints(x2[v, :m]))]
        if pre:
            a = [s * t % FR for s, t in zip(a, pre)]
        a = pyref.ntt(a, w)
        post = post_of(case, v)
        if post != "none":
            a = [s * t % FR for s, t in zip(a, tables[post])]
        if sub is not None:
            a = [(s - t) % FR for s, t in zip(a, F.limbs_to_ints(sub[v, :m]))]
        out.append(F.ints_to_limbs(a))
    return np.stack(out)


_FR_LIMBS = F.ints_to_limbs([FR])[0]


def fr_sub_limbs(a, b):
    """(a - b) mod r on (n, 4) limb arrays of canonical values, with numpy"""
    out, borrow = np.empty_like(a), np.zeros(a.shape[0], dtype=bool)
    for l in range(4):
        d = a[:, l] - b[:, l]
        under = a[:, l] < b[:, l]
        out[:, l] = d - borrow.astype(np.uint64)
        borrow = under | ((d == 0) & borrow)
    carry = np.zeros(a.shape[0], dtype=bool)
    for l in range(4):
        add = np.where(borrow, _FR_LIMBS[l], np.uint64(0)).astype(np.uint64)
        s = out[:, l] + add
        c1 = s < add
        s2 = s + carry.astype(np.uint64)
        carry = c1 | (s2 < s)
        out[:, l] = s2
    return out


def below_modulus(a):
    """elementwise a < r on (..., 4) limb arrays"""
    less, equal = np.zeros(a.shape[:-1], dtype=bool), np.ones(a.shape[:-1], dtype=bool)
    for l in (3, 2, 1, 0):
        less |= equal & (a[..., l] < _FR_LIMBS[l])
        equal &= a[..., l] == _FR_LIMBS[l]
    return less


def _self_check_sub():
    rng = np.random.default_rng(7)
    vals = [0, 1, FR - 1, FR - 2, (1 << 64) - 1, 1 << 64, 1 << 128, (1 << 192) - 1] + [int.from_bytes(rng.bytes(31), "little") for _ in range(24)]
    pairs = [(s, t) for s in vals for t in vals]
    got = fr_sub_limbs(F.ints_to_limbs([s for s, _ in pairs]), F.ints_to_limbs([t for _, t in pairs]))
    assert F.limbs_to_ints(got) == [(s - t) % FR for s, t in pairs]


_self_check_sub()


def oracle_mul(oracle, a, b):
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    out = np.empty_like(a)
    p = lambda t: t.ctypes.data_as(C.POINTER(C.c_uint64))
    oracle.lib().orc_fr_mul(p(out), p(a), p(b), C.c_size_t(a.shape[0]))
    return out


def geometric_limbs(oracle, s, b, m):
    """(m, 4) Montgomery limbs of s b^i: Python gives the factors b^n, the oracle's field product doubles the table"""
    t = np.empty((m, 4), dtype=np.uint64)
    t[0] = F.fr_to_mont([s])[0]
    n = 1
    while n < m:
        t[n:2 * n] = oracle_mul(oracle, t[:n], np.broadcast_to(F.fr_to_mont([pow(b, n, FR)])[0], (n, 4)))
        n *= 2
    return t


def reference_oracle(oracle, case, x, x2, sub):
    """the same with the oracle's transform (orc_ntt: plain forward, or inverse with its 1 / m) and orc_fr_mul"""
    m = 1 << case.logm
    assert case.data != "loose", "the oracle takes canonical words: loose inputs go to reference_ints, which reduces them"
    pre = geometric_limbs(oracle, 1, G, m) if case.pre == "coset_fwd" else None
    undo = m if case.inverse else 1                                  # the oracle's inverse transform has divided by m already
    tables = {}
    for name in {post_of(case, v) for v in range(case.batch)}:
        if name != "none":
            s, b = scale_of(name, m)
            tables[name] = geometric_limbs(oracle, s * undo, b, m)
        elif case.inverse:
            tables[name] = geometric_limbs(oracle, undo, 1, m)
    out = []
    for v in range(case.batch):
        a = x[v, :m]
        if x2 is not None:
            a = oracle_mul(oracle, a, x2[v, :m])
        if pre is not None:
            a = oracle_mul(oracle, a, pre)
        a = oracle.ntt(a, case.logm, inverse=case.inverse, coset=False)
        post = post_of(case, v)
        if post in tables:
            a = oracle_mul(oracle, a, tables[post])
        if sub is not None:
            a = fr_sub_limbs(a, sub[v, :m])
        out.append(a)
    return np.stack(out)


def check_ntt_case(zk, oracle, name):
    case = cases.NTT_CASES[name]
    m = 1 << case.logm
    assert cases.passes(case.logm) == cases.PLAN[case.logm]
    x, x2, sub, before = cases.ntt_inputs(case)
    got = zk.ntt_probe(x, case.logm, out=before, inverse=case.inverse, pre=case.pre, post=case.post, post_alt=case.post_alt,
                       alt_from=case.alt_from, in2=x2, sub=sub)
    assert (before == cases.SENTINEL).all()                          # (the wrapper works on a copy)
    if case.logm < ORACLE_FROM:
        want = reference_ints(case, x, x2, sub)
    else:
        want = reference_oracle(oracle, case, x, x2, sub)
    assert below_modulus(want).all(), (name, "the reference is not canonical")
    if case.data == "loose":                                         # the case is what it is named for: words in [r, 2r) go in
        n = cases.loose_words(case.logm)
        assert not below_modulus(x[:, :n]).any() and below_modulus(x[:, n:m]).all() and case.post == "none" and not case.inverse
    first_difference(got[:, :m], want, name)
    gaps = got[:, m:]
    assert (gaps == cases.SENTINEL).all(), (name, "the words behind vector %d were written" % int(np.argwhere((gaps != cases.SENTINEL).any(axis=(1, 2)))[0][0]))


def check_references_agree(oracle):
    """the two references on one size that both can do, every fused step in use"""
    for name in ("l12_everything_b2_alt1", "l10_abc_inverse_b3_alt2_structured", "l11_to_coset_b5_altnone_structured"):
        case = cases.NTT_CASES[name]
        x, x2, sub, _ = cases.ntt_inputs(case)
        first_difference(reference_oracle(oracle, case, x, x2, sub), reference_ints(case, x, x2, sub), "references, " + name)


def check_ntt_refusals(zk):
    m, logm = 8, 3
    x = np.zeros((2, m, 4), dtype=np.uint64)
    out = np.full((2, m, 4), 0xdeadbeef, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))
    u = C.c_uint32

    def call(in_=x, in2=None, sub=None, o=out, logm_=logm, batch=2, stride=m, post=1, post_alt=0, pre=0):
        return zk._lib.zk_ntt_probe(p(in_), p(in2), p(sub), p(o), u(logm_), u(batch), u(stride), 1, pre, post, post_alt, u(0), 0)
    assert call(stride=m - 1) == ZK_ERR_ARG
    assert call(batch=0) == ZK_ERR_ARG
    assert call(logm_=29) == ZK_ERR_ARG
    assert call(in_=None) == ZK_ERR_ARG
    assert call(o=None) == ZK_ERR_ARG
    assert call(sub=x, post=0) == ZK_ERR_ARG                         # sub without post
    assert call(sub=x, post=0, post_alt=1) == ZK_ERR_ARG
    assert call(post=6) == ZK_ERR_ARG and call(post_alt=-1) == ZK_ERR_ARG and call(pre=2) == ZK_ERR_ARG
    assert (out == 0xdeadbeef).all()                                 # a refused call writes nothing
    with pytest.raises(zk.ZkError) as e:
        zk.ntt_probe(x, 4)
    assert e.value.code == ZK_ERR_ARG and "stride" in str(e.value)
    assert call(sub=x, post=1) == 0 and not (out == 0xdeadbeef).any()   # ... and the same call with post is accepted: zeros in, zeros out
    assert not out.any()


# ---------------------------------------------------------------- (c), (d), (e): the pipeline of a batch
@functools.lru_cache(maxsize=None)
def h_reference(name, label):
    """every step of the H pipeline for one witness as VALUES (integers mod r), from Python dot products and pyref's transforms:
    ag, bg: coefficients of A, B times g^i; cz: coefficients of C times 1 / Z(g); ea, eb: A, B on the coset; p = ea eb;
    h = (icosetFFT(p) - C) / Z(g), m coefficients; parts[x] = (sum w^j p_j, sum w^j c_j) over j in [2048 x, 2048 (x + 1))"""
    s = cases.system(name)
    r, w = s.r1cs, s.witnesses[label]
    m = r.domain_size
    dot = lambda row: sum(c * w[i] for i, c in row) % FR
    rows = []
    for q, rr in enumerate((s.rows_a, s.rows_b, s.rows_c)):
        v = [dot(row) for row in rr] + (list(w[:r.nIn + 1]) if q == 0 else [])
        rows.append(v + [0] * (m - len(v)))
    om, gi = pyref.omega(m), pow(G, -1, FR)
    zinv = pow(pow(G, m, FR) - 1, -1, FR)
    gpow, gipow = geometric(1, G, m), geometric(1, gi, m)
    ag, bg = ([c * t % FR for c, t in zip(pyref.intt(v), gpow)] for v in rows[:2])
    cz = [c * zinv % FR for c in pyref.intt(rows[2])]
    ea, eb = pyref.ntt(ag, om), pyref.ntt(bg, om)
    p = [a * b % FR for a, b in zip(ea, eb)]
    h = [(q * t % FR * zinv - c) % FR for q, t, c in zip(pyref.intt(p), gipow, cz)]
    wpow = geometric(1, om, m)
    parts = [(sum(t * v for t, v in zip(wpow[x:x + 2048], p[x:x + 2048])) % FR, sum(t * v for t, v in zip(wpow[x:x + 2048], rows[2][x:x + 2048])) % FR)
             for x in range(0, m, 2048)]
    return dict(ag=ag, bg=bg, cz=cz, ea=ea, eb=eb, p=p, h=h, parts=parts, tail=h[m - 1])


@functools.lru_cache(maxsize=None)
def witness_limbs(name, label):
    a = F.fr_to_mont(cases.system(name).witnesses[label])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_key(oracle, name):
    return oracle.keygen(cases.system(name).r1cs, seed=2000 + len(name))[0]


@functools.lru_cache(maxsize=None)
def oracle_proofs(oracle, name):
    return tuple(oracle.prove(oracle_key(oracle, name), cases.system(name).r1cs, witness_limbs(name, l))[0] for l in cases.BATCHES["k3"])


_contexts = {}


def context(zk, oracle, monkeypatch, name, six):
    """the context of a system, max_batch = 3, made once per library and pipeline and shared by the checks; release() closes them"""
    key = (zk._lib_path_loaded, name, bool(six))
    if key not in _contexts:
        pk = zk.ProvingKey.from_parts(**oracle_key(oracle, name).parts())
        if six:
            monkeypatch.setenv("ZK_SIX_TRANSFORMS", "1")             # read when the context is created
        else:
            monkeypatch.delenv("ZK_SIX_TRANSFORMS", raising=False)
        ctx = zk.ProverContext(pk, cases.system(name).r1cs, max_batch=3)
        assert bool(ctx.info()["four_transforms"]) == (not six)
        _contexts[key] = (ctx, pk)
    return _contexts[key][0]


def release(zk):
    for key in [k for k in _contexts if k[0] == zk._lib_path_loaded]:
        ctx, pk = _contexts.pop(key)
        ctx.close(); pk.close()


def check_reference_against_oracle(oracle, name):
    """the second opinion: the oracle's witness map gives the same h -- h[m-1] of the unsatisfied witness included, which is not zero"""
    r = cases.system(name).r1cs
    m = r.domain_size
    for label in ("a", "b", "c", "bad"):
        ref = h_reference(name, label)
        h = oracle.witness_map(r, witness_limbs(name, label))
        first_difference(h[None, :m], F.ints_to_limbs(mont(ref["h"]))[None], "oracle's h against the reference, %s %s" % (name, label), "coefficient")
        assert (ref["tail"] != 0) == (label == "bad"), (name, label, "precondition: h[m-1] of the perturbed witness is not zero (pick another witness seed)")


def check_h_stages(zk, oracle, monkeypatch, name, batch, six):
    labels = cases.BATCHES[batch]
    k, m = len(labels), cases.DOMAIN[name]
    ctx = context(zk, oracle, monkeypatch, name, six)
    res = ctx.probe_h(np.stack([witness_limbs(name, l) for l in labels]))
    four = not six
    assert res["four"] == four and res["m"] == m and res["k"] == k and res["grid"] == (cases.GRID[name] if four else 0), {q: res[q] for q in ("four", "m", "k", "grid")}
    refs = [h_reference(name, l) for l in labels]
    for ref, label in zip(refs, labels):
        assert (ref["tail"] != 0) == (label == "bad"), (name, label)
    where = "%s %s %s" % (name, batch, "four" if four else "six")
    limbs = lambda lists: np.stack([F.ints_to_limbs(v) for v in lists])
    b_words = (lambda v: v) if four else mont                       # four transforms: B's vectors are canonical (its post-scale carries 1 / R)
    # after the first transform: vectors [A: k][B: k] (and [C: k])
    want = [mont(ref["ag"]) for ref in refs] + [b_words(ref["bg"]) for ref in refs] + ([] if four else [mont(ref["cz"]) for ref in refs])
    got = res["first"].reshape(-1, m, 4)
    first_difference(got, limbs(want), where + ", after the first transform (vector = group * k + proof; groups A, B%s)" % ("" if four else ", C"), "coefficient")
    # after the second: A and B on the coset
    want = [mont(ref["ea"]) for ref in refs] + [b_words(ref["eb"]) for ref in refs]
    first_difference(res["coset"].reshape(-1, m, 4), limbs(want), where + ", on the coset (vector = group * k + proof; groups A, B)", "point")
    # after the last step
    tails = limbs([mont([ref["tail"] for ref in refs])])[0]
    if four:
        first_difference(res["last"], limbs([ref["p"] for ref in refs]), where + ", p_j (vector = proof)", "point")
        want = [[v for sp, sc in ref["parts"] for v in (sp, sc * F.MONT_R % FR)] for ref in refs]
        first_difference(res["hpart"].reshape(k, -1, 4), limbs(want), where + ", d_hpart (vector = proof; element 2 x: sum of w^j p_j of workgroup x, 2 x + 1: of w^j c_j)", "element")
        first_difference(res["tail"][None], tails[None], where + ", d_tail", "proof")
    else:
        first_difference(res["last"], limbs([mont(ref["h"]) for ref in refs]), where + ", h (vector = proof)", "coefficient")
        assert res["hpart"] is None and res["tail"] is None
    first_difference(res["h_tail"][None], tails[None], where + ", h_tail", "proof")
    zero = [not row.any() for row in res["h_tail"]]
    assert zero == [l != "bad" for l in labels], (where, zero)


def check_degree_refusal(zk, oracle, monkeypatch, name, six):
    """ZK_ERR_DEGREE for the batch with the wrong middle witness -- whose h_tail check_h_stages compares by value --, then the good batch"""
    ctx = context(zk, oracle, monkeypatch, name, six)
    assert h_reference(name, "bad")["tail"] != 0 and all(h_reference(name, l)["tail"] == 0 for l in "abc")
    with pytest.raises(zk.ZkError) as e:
        zk.prove_batch(ctx, np.stack([witness_limbs(name, l) for l in cases.BATCHES["k3_bad_middle"]]))
    assert e.value.code == ZK_ERR_DEGREE, (name, six, e.value)
    got = zk.prove_batch(ctx, np.stack([witness_limbs(name, l) for l in cases.BATCHES["k3"]]))
    assert got == list(oracle_proofs(oracle, name)), (name, six, "the good batch after the refusal")


def check_h_refusals(zk, oracle, monkeypatch, six):
    name = "m256"
    r, m = cases.system(name).r1cs, cases.DOMAIN[name]
    ctx = context(zk, oracle, monkeypatch, name, six)                # max_batch = 3
    wm = witness_limbs(name, "a")
    two, four_w = np.stack([wm, witness_limbs(name, "b")]), np.stack([wm] * 4)
    names = ("first", "coset", "last", "hpart", "tail", "h_tail")
    bufs = {"first": np.zeros((3, 4, m, 4), dtype=np.uint64), "coset": np.zeros((2, 4, m, 4), dtype=np.uint64), "last": np.zeros((4, m, 4), dtype=np.uint64),
            "hpart": np.zeros((4, 1, 2, 4), dtype=np.uint64), "tail": np.zeros((4, 4), dtype=np.uint64), "h_tail": np.zeros((4, 4), dtype=np.uint64)}
    info = np.zeros(8, dtype=np.uint32)
    for b in list(bufs.values()) + [info]:
        b[...] = 0xdeadbeef
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))

    def probe(w, k, handle=ctx._h, missing=None):
        args = [None if q == missing else p(bufs[q]) for q in names]
        return zk._lib.zk_ctx_probe_h(handle, None if missing == "w" else p(w), C.c_uint32(k), 0, *args,
                                      None if missing == "info" else info.ctypes.data_as(C.POINTER(C.c_uint32)))
    untouched = lambda: all((b == 0xdeadbeef).all() for b in list(bufs.values()) + [info])
    assert probe(two, 0) == ZK_ERR_ARG                               # k = 0
    assert probe(four_w, 4) == ZK_ERR_ARG                            # k > max_batch
    assert probe(two, 1, handle=None) == ZK_ERR_ARG
    for missing in ("w", "info") + names:
        assert probe(two, 1, missing=missing) == ZK_ERR_ARG, missing
    assert untouched()
    expect = oracle_proofs(oracle, name)[0]
    ctx.submit(wm)
    try:
        assert probe(two, 2) == ZK_ERR_ARG                           # a proof is in flight
        with pytest.raises(zk.ZkError) as e:
            ctx.probe_h(two)
        assert e.value.code == ZK_ERR_ARG and "in flight" in str(e.value)
        assert untouched()                                           # a refused probe writes nothing
    finally:
        part, _ = ctx.collect()
    assert zk.proof_to_json(ctx.prove_combine(part), wm[1:1 + r.nIn]) == expect          # the refused probes did not disturb the proof in flight
    assert probe(two, 2) == 0 and not untouched()
    assert zk.prove(ctx, wm) == expect                               # a probe leaves the context as it was
