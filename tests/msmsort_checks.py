"""The checks behind test_msmsort_emul.py (CPU emulation build) and test_msmsort_gpu.py (device): the bucket sort of the multi-scalar
multiplications (msm_digit, k_sort_count / colscan / binscan / partition / partition_staged / fine) seen through zk_msm_sort_probe, against
a reference made of Python integers.

  (a) check_sort      for every case of msmsort_cases.py: the info block equals the Python restatement of the window and sort shape;
                      off[0] = 0, off non-decreasing, off[nb_total] = the number of non-zero digits; off[] equals the reference exactly;
                      every bucket's entries, sorted, equal the reference's (the order inside a bucket comes from LDS atomics and is not
                      part of the contract).  Montgomery and canonical input give the same sort.  A failure names bucket, proof, window,
                      digit and scalar of the first difference.
  (b) check_refusals  null pointers, batch = 0, too small an output, more buckets than the sort has.
  (c) check_msm       msm(bases, scalars, c) against the oracle's multi-exponentiation with the edge scalars of that c: ties the sign bit
                      and the carries of the sort to what k_msm_accumulate does with them.
`zk` is ethsnarks_amd.prover with the library under test loaded."""
import ctypes as C
import numpy as np
from ethsnarks_amd import fields as F
from helpers import tiled_bases
import msmsort_cases as cases

ZK_ERR_ARG = 1
SIGN = 1 << 31
_REF, _LIMBS = {}, {}


def reference(case):
    """(buckets, payloads) of every non-zero digit of the case, ordered by (bucket, payload), as uint32 arrays; computed once per case"""
    key = (case.scalars, case.n, case.c_used, case.plog, case.kbits)
    if key not in _REF:
        c, plog, n, kbits, nbp = case.c_used, case.plog, case.n, case.kbits, case.nbp
        plane_mask = (1 << plog) - 1
        digits = {}
        bk, pl = [], []
        for p, proof in enumerate(case.sorted_scalars()):
            for il, s in enumerate(proof):
                if s not in digits:
                    digits[s] = cases.signed_digits(s, c)
                for w, d in enumerate(digits[s]):
                    if d:
                        row = w >> plog
                        bk.append(((p << plog) | (w & plane_mask)) * nbp + abs(d) - 1)
                        pl.append(((row << kbits) | il if kbits else row * n + il) | (SIGN if d < 0 else 0))
        bk, pl = np.array(bk, dtype=np.uint32), np.array(pl, dtype=np.uint32)
        order = np.lexsort((pl, bk))
        _REF[key] = (bk[order], pl[order])
    return _REF[key]


def limbs(case, form):
    key = (case.scalars, form)
    if key not in _LIMBS:
        flat = [v for p in case.scalars for v in p]
        a = F.fr_to_mont(flat) if form == "mont" else F.ints_to_limbs(flat)
        _LIMBS[key] = a.reshape(case.batch, case.stride, 4)
    return _LIMBS[key]


def describe(case, bucket, payload=None):
    """what a bucket (and an entry) of the sort stands for"""
    S = 1 << case.plog
    bset, mag = divmod(int(bucket), case.nbp)
    text = "bucket %d = proof %d, plane %d, |digit| %d" % (bucket, bset >> case.plog, bset & (S - 1), mag + 1)
    if payload is not None:
        idx = int(payload) & (SIGN - 1)
        row, il = (idx >> case.kbits, idx & ((1 << case.kbits) - 1)) if case.kbits else divmod(idx, max(case.n, 1))
        w, p = (row << case.plog) | (bset & (S - 1)), bset >> case.plog
        text += "; entry 0x%08x = window %d (row %d), scalar %d, sign %s" % (int(payload), w, row, il, "-" if int(payload) & SIGN else "+")
        if p < case.batch and il < case.n:
            s = case.scalars[p][il]
            text += "; that scalar is %s = 0x%x" % (cases.label_of(case.c_used, s), s)
            if w < case.W:
                text += ", whose digit there is %d" % cases.signed_digits(s, case.c_used)[w]
    return text


def compare(case, off, got, info, form):
    tag = "%s (%s input)" % (case.name, form)
    want_b, want_p = reference(case)
    shape = {k: v for k, v in info.items() if k != "entries"}
    assert shape == case.info(), "%s: info block %r, the restated shape gives %r" % (tag, shape, case.info())
    nb = case.nb_total
    assert len(off) == nb + 1 and off[0] == 0, "%s: off[0] = %d" % (tag, off[0])
    off = off.astype(np.int64)
    down = np.flatnonzero(np.diff(off) < 0)
    assert down.size == 0, "%s: off decreases behind %s: %d -> %d" % (tag, describe(case, down[0]), off[down[0]], off[down[0] + 1])
    want_off = np.concatenate([[0], np.cumsum(np.bincount(want_b, minlength=nb))])
    bad = np.flatnonzero(off != want_off)
    if bad.size:
        b = max(int(bad[0]) - 1, 0)                                       # the first bucket whose COUNT differs ends at the first wrong offset
        raise AssertionError("%s: off[%d] = %d, reference %d: %s holds %d entries, reference %d" % (
            tag, bad[0], off[bad[0]], want_off[bad[0]], describe(case, b), off[b + 1] - off[b], want_off[b + 1] - want_off[b]))
    assert off[nb] == len(want_b) == len(got) == info["entries"], "%s: off[nb_total] = %d, info says %d entries, the scalars have %d non-zero digits" % (tag, off[nb], info["entries"], len(want_b))
    got_b = np.repeat(np.arange(nb, dtype=np.uint32), np.diff(off))       # (equal to want_b now: the offsets agree)
    got_p = got[np.lexsort((got, got_b))]
    bad = np.flatnonzero(got_p != want_p)
    if bad.size:
        e = int(bad[0])
        raise AssertionError("%s: entry %d of the sorted bucket contents differs.  got: %s\n  reference: %s" % (
            tag, e, describe(case, want_b[e], got_p[e]), describe(case, want_b[e], want_p[e])))
    if not len(want_b):
        assert not off.any(), "%s: no entries, but off is not all zero" % tag


def check_sort(zk, name, monkeypatch):
    case = cases.CASES[name]
    monkeypatch.delenv("ZK_SORT_PER_GROUP", raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    for form in case.forms:
        off, got, info = zk.msm_sort_probe(limbs(case, form), n=case.n, c=case.c, plog=case.plog, shift_payload=case.shift, canonical=form == "canon")
        compare(case, off, got, info, form)


def check_refusals(zk, monkeypatch):
    monkeypatch.delenv("ZK_SORT_PER_GROUP", raising=False)
    case = cases.CASES["three_groups_c13"]
    s = limbs(case, "mont")
    u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    off, out, info = np.zeros(case.nb_total + 1, dtype=np.uint32), np.full(case.n * case.W + 1, 0xdeadbeef, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    p32 = lambda a: a.ctypes.data_as(u32)

    def probe(scalars=s.ctypes.data_as(u64), n=case.n, batch=1, stride=case.n, c=13, plog=0, off_p=p32(off), off_cap=off.size, out_p=p32(out), out_cap=out.size, info_p=p32(info)):
        return zk._lib.zk_msm_sort_probe(scalars, C.c_uint32(n), C.c_uint32(batch), C.c_uint32(stride), 0, C.c_uint32(c), C.c_uint32(plog), 0, 0,
                                         off_p, C.c_uint64(off_cap), out_p, C.c_uint64(out_cap), info_p)

    assert probe(scalars=None) == ZK_ERR_ARG and probe(off_p=None) == ZK_ERR_ARG and probe(out_p=None) == ZK_ERR_ARG and probe(info_p=None) == ZK_ERR_ARG
    assert probe(batch=0) == ZK_ERR_ARG
    assert probe(stride=case.n - 1) == ZK_ERR_ARG
    assert probe(plog=8) == ZK_ERR_ARG
    assert probe(off_cap=case.nb_total) == ZK_ERR_ARG
    # too small an output: refused, the entry count reported, nothing written
    entries = len(reference(case)[0])
    assert probe(out_cap=entries - 1) == ZK_ERR_ARG
    assert int(info[10]) == entries and (out == 0xdeadbeef).all()
    # three proofs of 2^19 buckets are more than the sort's 2^20
    three = np.ascontiguousarray(np.broadcast_to(s[0, :8], (3, 8, 4)))
    big_off, big_out = np.zeros((4 << 19) + 1, dtype=np.uint32), np.zeros(3 * 8 * 13, dtype=np.uint32)      # (room for the answer, were it given)
    big = dict(scalars=three.ctypes.data_as(u64), n=8, stride=8, c=20, off_p=p32(big_off), off_cap=big_off.size, out_p=p32(big_out), out_cap=big_out.size)
    assert probe(batch=3, **big) == ZK_ERR_ARG
    assert b"batch too large" in zk._lib.zk_last_error()
    assert probe(batch=1, plog=2, **big) == ZK_ERR_ARG
    assert b"batch too large" in zk._lib.zk_last_error()    # ... and the next call is answered
    assert probe(out_cap=entries) == 0
    compare(case, off.copy(), out[:entries].copy(), dict(zip(zk.SORT_INFO, (int(v) for v in info))), "mont")


_BASES = {}


def msm_inputs(oracle, c, g2):
    """the edge scalars of width c over MSM_DISTINCT distinct bases, tiled, then P, -P under 3, 3 and Q, Q under 4, 4"""
    if g2 not in _BASES:
        k = 8 if g2 else 4                                                # limbs (u64) of one coordinate
        pts = oracle.batch_mul(F.fr_to_mont([5, 9]), g2=g2)
        neg = pts[0].copy()
        neg[k:2 * k] = F.fq_to_mont([(-v) % F.FQ for v in F.fq_from_mont(neg[k:2 * k].reshape(-1, 4))]).reshape(-1)
        _BASES[g2] = (tiled_bases(oracle, len(cases.msm_scalars(2)) - 4, g2=g2, distinct=cases.MSM_DISTINCT), np.stack([pts[0], neg, pts[1], pts[1]]))
    sc = cases.msm_scalars(c)
    tiled, special = _BASES[g2]
    assert len(tiled) == len(sc) - 4
    return np.concatenate([tiled, special]), F.fr_to_mont(sc)


def check_msm(zk, oracle, c, g2, monkeypatch):
    monkeypatch.delenv("ZK_SORT_PER_GROUP", raising=False)
    bases, s = msm_inputs(oracle, c, g2)
    got, want = zk.msm(bases, s, g2=g2, c=c), oracle.msm(bases, s, g2=g2)
    assert np.array_equal(got, want), "%s multi-exponentiation of the edge scalars at c = %d differs from the oracle's" % ("G2" if g2 else "G1", c)
