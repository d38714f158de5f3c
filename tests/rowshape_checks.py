"""Checks of the R1CS row evaluation on the systems of rowshape_cases.py.  They run unchanged on the CPU stand-in (test_rowshape_emul.py) and
on the device (test_rowshape_gpu.py); `zk` is the ethsnarks_amd.prover module with a library loaded, `oracle` the CPU oracle's binding.
Everything is integer arithmetic and every comparison is bit-exact: there is no tolerance anywhere.

  (a) check_rows          zk_ctx_probe_rows against Python dot products, every row of every matrix of every proof, padding and input rows
  (b) check_witness_map   ctx.witness_map against the oracle's, and against pyref's where the domain is small
  (c) check_proofs        proof bytes against the oracle's, with four and with six transforms, one at a time and as a batch
  (d) check_refusal       a witness entry that only a later chunk of a long row reads, perturbed: ZK_ERR_DEGREE exactly when the oracle's h[m-1] != 0
  (e) check_probe_refusals  the probe's own argument checks"""
import contextlib
import functools
import os
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import rowshape_cases as cases

ZK_ERR_ARG, ZK_ERR_DEGREE = 1, 7
MATRIX = "ABC"


@functools.lru_cache(maxsize=None)
def mont(name, label):
    a = F.fr_to_mont(cases.witnesses(name)[label])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_rows(name, label):
    """[A, B, C][row of the domain] as integers: <M_j, w> mod r for j < nC; then A continues with w[0 .. nIn] (the input-consistency rows);
    everything else up to the domain size is 0.  Computed once per (case, witness)."""
    s = cases.system(name)
    r, w = s.r1cs, cases.witnesses(name)[label]
    m = r.domain_size
    out = []
    for q, rows in enumerate((s.rows_a, s.rows_b, s.rows_c)):
        v = [cases.dot(row, w) for row in rows]
        if q == 0:
            v += w[:r.nIn + 1]
        out.append(tuple(v + [0] * (m - len(v))))
        assert len(out[-1]) == m
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_key(oracle, name):
    return oracle.keygen(cases.system(name).r1cs, seed=1000 + len(name))[0]


@contextlib.contextmanager
def transforms(six):
    """ZK_SIX_TRANSFORMS=1 while a context is created (it is read there): the six-transform H pipeline instead of the default four"""
    old = os.environ.get("ZK_SIX_TRANSFORMS")
    if six:
        os.environ["ZK_SIX_TRANSFORMS"] = "1"
    else:
        os.environ.pop("ZK_SIX_TRANSFORMS", None)
    try:
        yield
    finally:
        os.environ.pop("ZK_SIX_TRANSFORMS", None)
        if old is not None:
            os.environ["ZK_SIX_TRANSFORMS"] = old


_contexts = {}


def context(zk, oracle, name, six=False):
    """the context of a case, max_batch = 3, made once per library and path and shared by the checks (the four-transform tables cost a group
    operation per non-zero of C when they are built); release() closes them"""
    key = (zk._lib_path_loaded, name, bool(six))
    if key not in _contexts:
        pk = zk.ProvingKey.from_parts(**oracle_key(oracle, name).parts())
        with transforms(six):
            ctx = zk.ProverContext(pk, cases.system(name).r1cs, max_batch=3)
        assert bool(ctx.info()["four_transforms"]) == (not six)
        _contexts[key] = (ctx, pk)
    return _contexts[key][0]


def release(zk):
    for key in [k for k in _contexts if k[0] == zk._lib_path_loaded]:
        ctx, pk = _contexts.pop(key)
        ctx.close(); pk.close()


def compare_rows(got, name, labels, where):
    """got: (3, k, m, 4) raw limbs from the probe; the first mismatch is named by matrix, proof and row"""
    r = cases.system(name).r1cs
    m = r.domain_size
    assert got.shape == (3, len(labels), m, 4), (where, got.shape)
    raw = F.limbs_to_ints(got)
    # The first transform loads these words into loose butterflies, which accept [0, 2r) (csrc/ntt.hpp k_ntt_pass, csrc/bn254.hpp "loose
    # domain"); the four-transform path also hands the C rows to strict sums (k_hl_product), which accept [0, r) only.  The row kernels
    # compute with the strict Fr::add / Fr::mul and copy canonical witness words, so CANONICAL [0, r) -- inside both -- is what must hold.
    loose = [i for i, v in enumerate(raw) if v >= F.FR]
    assert not loose, (where, "not canonical: matrix %s, proof %d, row %d" % (MATRIX[loose[0] // (len(labels) * m)], loose[0] // m % len(labels), loose[0] % m), hex(raw[loose[0]]))
    values = [v * F.FR_RINV % F.FR for v in raw]
    for q in range(3):
        for p, label in enumerate(labels):
            at = (q * len(labels) + p) * m
            want = expected_rows(name, label)[q]
            if tuple(values[at:at + m]) != want:
                bad = [j for j in range(m) if values[at + j] != want[j]]
                kind = "row" if bad[0] < r.nC else "input row" if q == 0 and bad[0] <= r.nC + r.nIn else "padding row"
                pytest.fail("%s: matrix %s, proof %d (%s), %s %d is wrong (%d rows of this vector are): got %#x, expected %#x"
                            % (where, MATRIX[q], p, label, kind, bad[0], len(bad), values[at + bad[0]], want[bad[0]]))


BATCH = ("a", "alternate", "b")                                      # three distinct witnesses of one system, one of them an edge witness


def check_rows(zk, oracle, name, six=False, labels_list=(("a",), BATCH)):
    """six: probe a context made with ZK_SIX_TRANSFORMS=1 (the CPU stand-in: its tables are quick to build); the row evaluation is one helper
    under both pipelines"""
    ctx = context(zk, oracle, name, six)
    for labels in labels_list:
        w = np.stack([mont(name, l) for l in labels])
        compare_rows(ctx.probe_rows(w), name, labels, (name, "k = %d" % len(labels)))


def check_edge_witnesses(zk, oracle, name, six=False):
    """free variables all 0 and all r - 1; and witnesses again through canonical = 1: the same words come back"""
    ctx = context(zk, oracle, name, six)
    w = np.stack([mont(name, l) for l in ("zero", "rm1")])
    compare_rows(ctx.probe_rows(w), name, ("zero", "rm1"), (name, "edges"))
    for labels in (("rm1",), ("zero", "a", "rm1")):
        canon = np.stack([F.ints_to_limbs(cases.witnesses(name)[l]) for l in labels])
        compare_rows(ctx.probe_rows(canon, canonical=True), name, labels, (name, "canonical", labels))


def check_witness_map(zk, oracle, name, six=False, labels=("a", "alternate")):
    import pyref
    r = cases.system(name).r1cs
    ctx = context(zk, oracle, name, six)
    for label in labels:
        wm = mont(name, label)
        got = ctx.witness_map(wm)
        want = oracle.witness_map(r, wm)
        wrong = np.argwhere((got != want).any(axis=1))
        assert wrong.size == 0, (name, label, "first wrong coefficient of h", int(wrong[0][0]), "of", len(wrong))
        if r.domain_size <= 512 and label == labels[0]:                  # (the big-int map is quadratic)
            assert F.fr_from_mont(got) == pyref.witness_map(r.as_pyref(), cases.witnesses(name)[label]), (name, label, "pyref")


def check_proofs(zk, oracle, name, six):
    """proof bytes of the three witnesses, one at a time and as a batch, on the default path (four transforms) or with ZK_SIX_TRANSFORMS=1"""
    r = cases.system(name).r1cs
    pk_o = oracle_key(oracle, name)
    ws = [mont(name, l) for l in BATCH]
    expect = [oracle.prove(pk_o, r, w)[0] for w in ws]
    assert len(set(expect)) == len(expect)
    ctx = context(zk, oracle, name, six)
    singles = [zk.prove(ctx, w) for w in ws]
    for label, got, want in zip(BATCH, singles, expect):
        assert got == want, (name, label, "six" if six else "four")
    assert zk.prove_batch(ctx, np.stack(ws)) == singles, (name, "batch")


def check_refusal(zk, oracle, six):
    """the variable n_free of the "late" system stands at term SPMV_CHUNK + 5 of A's row 3 and nowhere else: a device that drops or
    misplaces the second chunk of that row accepts the perturbed witness, or refuses the good one"""
    name = "late"
    s = cases.system(name)
    r, m = s.r1cs, s.r1cs.domain_size
    good = cases.witnesses(name)["a"]
    bad = list(good); bad[s.n_free] = (bad[s.n_free] + 1) % F.FR
    gm, bm = mont(name, "a"), F.fr_to_mont(bad)
    assert not r.is_satisfied(bad)
    h_good, h_bad = oracle.witness_map(r, gm), oracle.witness_map(r, bm)
    assert not h_good[m - 1].any()
    refuse = bool(h_bad[m - 1].any())                                   # ZK_ERR_DEGREE exactly when the reference's h[m-1] != 0
    assert refuse, "precondition: the oracle's h[m-1] of the perturbed witness is non-zero (pick another cases.LATE_SEED)"
    expect = oracle.prove(oracle_key(oracle, name), r, gm)[0]
    ctx = context(zk, oracle, name, six)
    # the rows say where: the two witnesses differ in A's row 3 and nowhere else
    rows_good, rows_bad = ctx.probe_rows(gm), ctx.probe_rows(bm)
    compare_rows(rows_good, name, ("a",), (name, "good"))
    differ = np.argwhere((rows_good != rows_bad).any(axis=3)).tolist()
    assert differ == [[cases.LATE_ROW[0], 0, cases.LATE_ROW[1]]], differ
    got = F.limbs_to_ints(rows_bad[cases.LATE_ROW[0], 0, cases.LATE_ROW[1]])[0] * F.FR_RINV % F.FR
    assert got == cases.dot(s.rows_a[cases.LATE_ROW[1]], bad)
    with pytest.raises(zk.ZkError) as e:
        zk.prove(ctx, bm)
    assert e.value.code == ZK_ERR_DEGREE, (six, e.value)
    assert zk.prove(ctx, gm) == expect                                  # ... and the context proves on


def check_probe_refusals(zk, oracle, six=False):
    import ctypes as C
    name = "padding_250_5"
    r = cases.system(name).r1cs
    ctx = context(zk, oracle, name, six)                                # max_batch = 3
    wm = mont(name, "a")
    two, four = np.stack([wm, mont(name, "b")]), np.stack([wm] * 4)
    out = np.zeros((3, 4, r.domain_size, 4), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    probe = lambda w, k: zk._lib.zk_ctx_probe_rows(ctx._h, p(w), C.c_uint32(k), 0, p(out))
    out[:] = 0xdeadbeef
    assert probe(two, 0) == ZK_ERR_ARG                                  # k = 0
    assert probe(four, 4) == ZK_ERR_ARG                                 # k > max_batch
    assert zk._lib.zk_ctx_probe_rows(None, p(two), C.c_uint32(1), 0, p(out)) == ZK_ERR_ARG
    assert zk._lib.zk_ctx_probe_rows(ctx._h, None, C.c_uint32(1), 0, p(out)) == ZK_ERR_ARG
    assert zk._lib.zk_ctx_probe_rows(ctx._h, p(two), C.c_uint32(1), 0, None) == ZK_ERR_ARG
    ctx.submit(wm)
    try:
        assert probe(two, 1) == ZK_ERR_ARG                              # a proof is in flight
        with pytest.raises(zk.ZkError) as e:
            ctx.probe_rows(two)
        assert e.value.code == ZK_ERR_ARG and "in flight" in str(e.value)
        assert (out == 0xdeadbeef).all()                                # a refused probe writes nothing
    finally:
        part, _ = ctx.collect()
    expect = oracle.prove(oracle_key(oracle, name), r, wm)[0]
    assert zk.proof_to_json(ctx.prove_combine(part), wm[1:1 + r.nIn]) == expect          # the refused probes did not disturb the proof in flight
    compare_rows(ctx.probe_rows(two), name, ("a", "b"), (name, "after the refusals"))
    assert zk.prove(ctx, wm) == expect                                  # a probe leaves the context as it was
