"""The checks behind test_msmstage_emul.py (CPU emulation build) and test_msmstage_gpu.py (device): what every stage of a multi-scalar
multiplication leaves behind the bucket sort -- k_msm_precompute, k_msm_accumulate, k_msm_bucket_finalize / k_msm_heavy, k_msm_rowcol_sum,
k_msm_weighted_sum and MsmWork::finish -- seen through zk_msm_stage_probe, against a reference that cannot share a mistake with the kernels.

Every base is k_i G for a known integer k_i, so every value on the way is e G for an integer e mod r that Python integers give exactly:
  table       row rho, base i                    k_i 2^(c 2^plog rho)
  piece       chunk j, bucket b                  the signed sum of the table exponents of the DEVICE's sorted[begin .. end) entries that lie
                                                 in b (the order inside a bucket comes from LDS atomics and is not part of the contract, so
                                                 this one stage follows the device's entry order -- after off[] was compared exactly and
                                                 every bucket's entries, as a multiset, with msmsort_checks.reference)
  bucket      b                                  the sum over its digits, from the scalars alone (both MSMs of a merged tail)
  partial_a   set s: Row_hi, then Col_lo         sum_lo e_(hi L + lo), sum_hi e_(hi L + lo)
  partial_b   set s                              sum_b (b + 1) e_b
  result                                         sum_s 2^(c s) R_s, which must also be sum_i s_i k_i
  heavy_list                                     as a set, and its count: the buckets whose restated piece ranges hold more than MSM_HEAVY
The expected exponents become points through ONE oracle.batch_mul per case; a device value X, Y, ZZ, ZZZ means the affine point
(X / ZZ, Y / ZZZ), infinity iff ZZ = 0 mod q, and is compared with the expected (x, y) as X = x ZZ and Y = y ZZZ in Fq (Fq2) with ZZZ != 0 --
equality of field elements, no tolerance.  Separately every raw coordinate must lie below 2 q (the loose domain); the probe fills the
buffers with all-ones words before the launches, so a slot that a kernel should have written and did not fails this range check.
A failure names stage, set, bucket (hi, lo), piece and chunk, and the expected and found exponent class.
`zk` is ethsnarks_amd.prover with the library under test loaded."""
import ctypes as C
import numpy as np
from ethsnarks_amd import fields as F
import msmsort_checks as sort_chk
import msmstage_cases as cases

FR, FQ = F.FR, F.FQ
ZK_ERR_ARG = 1
SIGN = 1 << 31
RINV = pow(1 << 256, -1, FQ)
_Q_LIMBS = F.ints_to_limbs([FQ])[0]
_2Q_LIMBS = F.ints_to_limbs([2 * FQ])[0]


# ---- Fq / Fq2 on raw Montgomery integers
def _mm(a, b):
    return a * b * RINV % FQ


def _mul(g2, a, b):
    if not g2:
        return (_mm(a[0], b[0]),)
    return ((_mm(a[0], b[0]) - _mm(a[1], b[1])) % FQ, (_mm(a[0], b[1]) + _mm(a[1], b[0])) % FQ)          # u^2 = -1


def _zero(v):
    return all(x % FQ == 0 for x in v)


def _same(a, b):
    return all((x - y) % FQ == 0 for x, y in zip(a, b))


def below_2q(arr):
    """(..., 4) u64 limbs -> bool array: value < 2 q"""
    lt, eq = np.zeros(arr.shape[:-1], dtype=bool), np.ones(arr.shape[:-1], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (arr[..., k] < _2Q_LIMBS[k])
        eq &= arr[..., k] == _2Q_LIMBS[k]
    return lt


def zero_mod_q(arr):
    """(..., 4) limbs known to be < 2 q -> bool: the value is 0 or q"""
    return (arr == 0).all(axis=-1) | (arr == _Q_LIMBS).all(axis=-1)


class Expected:
    """exponent -> affine point (raw Montgomery coordinates), through one oracle.batch_mul"""

    def __init__(self, oracle, g2, exps):
        self.g2, self.w = g2, 2 if g2 else 1
        uniq = sorted({e % FR for e in exps} - {0})
        self.pt = {}
        if uniq:
            pts = oracle.batch_mul(F.fr_to_mont(uniq), g2=g2)
            vals = F.limbs_to_ints(pts)
            per = 2 * self.w
            for j, e in enumerate(uniq):
                v = vals[j * per:(j + 1) * per]
                self.pt[e] = (tuple(v[:self.w]), tuple(v[self.w:]))
        self.by_x = {p[0]: e for e, p in self.pt.items()}
        self.seen = {}

    def coords(self, raw):
        """one point (coordinates, 4) u64 -> tuple of coordinates, each a tuple of 1 | 2 ints"""
        v = F.limbs_to_ints(raw)
        return [tuple(v[k:k + self.w]) for k in range(0, len(v), self.w)]

    def classify(self, raw):
        """what a raw device point is, for a failure message"""
        c = self.coords(raw)
        if any(x >= 2 * FQ for co in c for x in co):
            return "out of range (a coordinate >= 2 q; all-ones words: never written)"
        if len(c) == 2:
            if _zero(c[0]) and _zero(c[1]):
                return "infinity"
            e = self.by_x.get(tuple(x % FQ for x in c[0]))
        else:
            if _zero(c[2]):
                return "infinity"
            if _zero(c[3]):
                return "not a point (ZZZ = 0, ZZ != 0)"
            e = next((e for e, p in self.pt.items() if _same(c[0], _mul(self.g2, p[0], c[2]))), None)
        if e is None:
            return "a point that is none of the case's expected ones"
        p = self.pt[e]
        ok = _same(c[1], p[1]) if len(c) == 2 else _same(c[1], _mul(self.g2, p[1], c[3]))
        return "exponent 0x%x" % e if ok else "exponent 0x%x (the negation of an expected point)" % (FR - e)

    def matches(self, raw, e):
        """raw device point == e G; equal (raw, e) pairs -- tiled bases, equal buckets -- are compared once"""
        key = (raw.tobytes(), e % FR)
        if key not in self.seen:
            self.seen[key] = self._matches(raw, e % FR)
        return self.seen[key]

    def _matches(self, raw, e):
        c = self.coords(raw)
        if len(c) == 2:
            return (_zero(c[0]) and _zero(c[1])) if e == 0 else (_same(c[0], self.pt[e][0]) and _same(c[1], self.pt[e][1]))
        if e == 0:
            return _zero(c[2])
        x, y = self.pt[e]
        return not _zero(c[2]) and not _zero(c[3]) and _same(c[0], _mul(self.g2, x, c[2])) and _same(c[1], _mul(self.g2, y, c[3]))


def exp_class(e):
    e %= FR
    return "infinity (exponent 0)" if e == 0 else "exponent 0x%x" % e


def where(case, b):
    nb, L = case.shape.nb, case.tail.L
    s, d = divmod(int(b), nb)
    return "set %d, bucket %d (hi %d, lo %d)" % (s, d, d // L, d % L)


def fail(case, stage, what, exp, raw, want):
    raise AssertionError("%s: stage %s: %s: expected %s, found %s" % (case.name, stage, what, exp_class(want), exp.classify(raw)))


def in_range(case, stage, arr, names):
    """every raw coordinate below 2 q -- a range assertion, separate from the values"""
    bad = np.argwhere(~below_2q(arr))
    assert bad.size == 0, "%s: stage %s: %s has a coordinate >= 2 q (first: %s of %d out of range; all-ones words = never written)" % (
        case.name, stage, names(bad[0]), tuple(int(v) for v in bad[0]), len(bad))


# ---- the reference exponents
class Reference:
    def __init__(self, case):
        self.case = case
        c, S = case.c_used, 1 << case.plog
        self.rowmul = [pow(2, c * S * rho, FR) for rho in range(case.shape.rows)]
        nbt = case.shape.nb * S
        self.bucket = [0] * nbt
        self.occupied = set()
        for m, srt in zip(case.msms(), case.sorts):
            bk, pl = sort_chk.reference(srt)
            for b, p in zip(bk.tolist(), pl.tolist()):
                self.bucket[b] = (self.bucket[b] + self.entry(m, srt, p)) % FR
                self.occupied.add(b)
        nb, L, H = case.shape.nb, case.tail.L, case.tail.H
        self.partial_a, self.partial_b = [], []
        for s in range(S):
            e = self.bucket[s * nb:(s + 1) * nb]
            self.partial_a += [sum(e[h * L:(h + 1) * L]) % FR for h in range(H)] + [sum(e[l::L]) % FR for l in range(L)]
            self.partial_b.append(sum((b + 1) * v for b, v in enumerate(e) if v) % FR)
        self.result = sum(pow(2, c * s, FR) * r for s, r in enumerate(self.partial_b)) % FR
        direct = 0
        for m in case.msms():
            for i, s in enumerate(m.scalars):
                k = m.base_of(i)
                if k is not None:
                    direct += s * m.ks[k]
        assert self.result == direct % FR, "%s: the reference's own stages do not add up to sum_i s_i k_i" % case.name

    def entry(self, m, srt, payload):
        """exponent of one sorted entry: sign * k_base * 2^(c 2^plog row), 0 when this MSM has no base for the scalar"""
        idx = payload & (SIGN - 1)
        row, i = (idx >> srt.kbits, idx & ((1 << srt.kbits) - 1)) if srt.kbits else divmod(idx, m.n_sort)
        k = m.base_of(i)
        if k is None:
            return 0
        e = m.ks[k] * self.rowmul[row] % FR
        return FR - e if payload & SIGN and e else e

    def table(self):
        return [[k * r % FR for k in self.case.first.ks] for r in self.rowmul]

    def pieces(self, side, off, got_sorted, rule):
        """{piece index: (exponent, chunk, bucket)} from the device's own entry order"""
        m, srt = self.case.msms()[side], self.case.sorts[side]
        total = int(off[-1])
        seg = rule.len(total)
        bucket_of = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
        out = {}
        for e in range(total):
            j, b = e // seg, int(bucket_of[e])
            cur = out.get(j + b, (0, j, b))
            assert cur[1:] == (j, b), "two (chunk, bucket) pairs share piece %d" % (j + b)
            out[j + b] = ((cur[0] + self.entry(m, srt, int(got_sorted[e]))) % FR, j, b)
        return out


def check_sorted(case, side, off, got):
    """off[] exactly, every bucket's entries as a multiset (msmsort_checks.reference)"""
    srt = case.sorts[side]
    want_b, want_p = sort_chk.reference(srt)
    nb = srt.nb_total
    tag = "%s: stage sort%s" % (case.name, " (second MSM)" if side else "")
    want_off = np.concatenate([[0], np.cumsum(np.bincount(want_b, minlength=nb))])
    bad = np.flatnonzero(off.astype(np.int64) != want_off)
    assert bad.size == 0, "%s: off[%d] = %d, reference %d (%s)" % (tag, bad[0], off[bad[0]], want_off[bad[0]], sort_chk.describe(srt, max(int(bad[0]) - 1, 0)))
    assert len(got) == len(want_p), "%s: %d entries, reference %d" % (tag, len(got), len(want_p))
    got_b = np.repeat(np.arange(nb, dtype=np.uint32), np.diff(want_off))
    got_p = got[np.lexsort((got, got_b))]
    bad = np.flatnonzero(got_p != want_p)
    assert bad.size == 0, "%s: entry %d of the sorted bucket contents differs.  got: %s\n  reference: %s" % (
        tag, bad[0], sort_chk.describe(srt, want_b[bad[0]], got_p[bad[0]]), sort_chk.describe(srt, want_b[bad[0]], want_p[bad[0]]))


def run(zk, case, monkeypatch):
    for k in ("ZK_MSM_QUAD", "ZK_MSM_QUAD_ACC", "ZK_ACC_PAIRS", "ZK_ROWCOL_SEG", "ZK_SEG_MIN", "ZK_SEG_MAX", "ZK_SORT_PER_GROUP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)

    def arg(m, bases):
        d = dict(bases=bases, scalars=F.fr_to_mont(m.scalars))
        if m.borrowed:
            d.update(n_src=m.n_sort, offset=m.offset, pos=m.pos, shift_payload=m.shift)
        return d
    return zk.msm_stage_probe(arg(case.first, case.bases[0]), arg(case.second, case.bases[1]) if case.second else None, g2=case.g2, c=case.c,
                              plog=case.plog, tail_lanes=case.tail_lanes)


def make_bases(oracle, case):
    """the bases k_i G of both MSMs (k = 0: the affine infinity, all-zero limbs), made once per case"""
    if not hasattr(case, "bases"):
        case.bases = []
        for m in case.msms():
            uniq = sorted(set(m.ks) - {0})
            pts = dict(zip(uniq, oracle.batch_mul(F.fr_to_mont(uniq), g2=case.g2))) if uniq else {}
            zero = np.zeros(16 if case.g2 else 8, dtype=np.uint64)
            case.bases.append(np.stack([pts[k] if k else zero for k in m.ks]))
    return case.bases


def check_case(zk, oracle, name, monkeypatch, emulated):
    case = cases.CASES[name]
    make_bases(oracle, case)
    got, info = run(zk, case, monkeypatch)
    sh = case.shape
    # ---- the shape the library used is the restated one; the slots are the machine's
    have = {k: info[k] for k in sh.info()}
    assert have == sh.info(), "%s: info block %r, the restated shape gives %r" % (name, have, sh.info())
    assert (info["MSM_HEAVY"], info["MSM_TREE"], info["MSM_HEAVY_GRID"]) == (cases.MSM_HEAVY, cases.MSM_TREE, cases.MSM_HEAVY_GRID)
    assert info["second"] == int(case.second is not None) and info["sort_kbits"] == case.sorts[0].kbits
    slots = [info["slots"]] + ([info["slots2"]] if case.second else [])
    if emulated:
        assert slots == [s.slots(True) for s in case.shapes], "%s: slots %r" % (name, slots)
    else:
        cus = zk.device_info()["compute_units"]
        assert slots == [s.slots(False, cus) for s in case.shapes], "%s: slots %r on %d CUs" % (name, slots, cus)
    if case.second:
        s2 = case.shapes[1]
        assert (info["seg_min2"], info["seg_max2"], info["acc_form2"]) == (s2.seg_min, s2.seg_max, s2.acc_form)
    case.reaches(slots, emulated)                                         # ... and on THIS machine the case is what it is named for
    rules = case.rules(slots)
    ref = Reference(case)
    # ---- sort (the order inside a bucket is the device's own)
    sides = [(0, got["off"], got["sorted"], got["pieces"], info["entries"], info["pieces"])]
    if case.second:
        sides.append((1, got["off2"], got["sorted2"], got["pieces2"], info["entries2"], info["pieces2"]))
    piece_ref = []
    for side, off, srt, _, entries, _ in sides:
        assert entries == len(srt) == int(off[-1])
        check_sorted(case, side, off, srt)
        piece_ref.append(ref.pieces(side, off, srt, rules[side]))
    # ---- every expected exponent -> one batch multiplication
    table = ref.table()
    exps = {e for row in table for e in row} | {v[0] for pr in piece_ref for v in pr.values()} | set(ref.bucket) | set(ref.partial_a) | set(ref.partial_b) | {ref.result}
    exp = Expected(oracle, case.g2, exps)
    # ---- table
    in_range(case, "table", got["table"], lambda ix: "row %d, base %d" % (ix[0], ix[1]))
    assert got["table"].shape[:2] == (sh.rows, case.first.n)
    for rho, row in enumerate(table):
        for i, e in enumerate(row):
            if not exp.matches(got["table"][rho, i], e):
                fail(case, "table (k_msm_precompute)", "row %d, base %d (k_i 2^(%d rho))" % (rho, i, case.c_used << case.plog), exp, got["table"][rho, i], e)
    # ---- pieces: every slot of every bucket's piece range is written, and holds the sum of its entries
    for (side, off, srt, pieces, _, n_pieces), pr, rule in zip(sides, piece_ref, rules):
        stage = "pieces%s (k_msm_accumulate)" % (" of the second MSM" if side else "")
        total, seg = int(off[-1]), rule.len(int(off[-1]))
        assert n_pieces == len(pieces) == ((-(-total // seg) + len(off) - 2) if total else 0), "%s: %s: %d pieces copied" % (name, stage, n_pieces)
        want_slots = set()
        for b in range(len(off) - 1):
            s0, s1 = cases.piece_range(off, rule, b)
            want_slots.update(range(s0, s1))
        assert want_slots == set(pr), "%s: %s: the restated piece ranges and the chunk walk name different slots" % (name, stage)
        for slot in sorted(pr):
            e, j, b = pr[slot]
            raw = pieces[slot]
            what = "piece %d = chunk %d (entries %d .. %d) in %s" % (slot, j, j * seg, min((j + 1) * seg, total) - 1, where(case, b))
            assert below_2q(raw).all(), "%s: stage %s: %s has a coordinate >= 2 q: %s" % (name, stage, what, exp.classify(raw))
            if not exp.matches(raw, e):
                fail(case, stage, what, exp, raw, e)
    # ---- the heavy list: count and set
    per = case.pieces_per_bucket(slots)
    want_heavy = case.heavy_set(slots)
    heavy = [int(b) for b in got["heavy_list"]]
    assert info["heavy_count"] == len(heavy) == len(want_heavy) and set(heavy) == want_heavy, "%s: stage heavy list (k_msm_bucket_finalize): %d queued %r, restated %r (pieces %r)" % (
        name, info["heavy_count"], sorted(heavy), sorted(want_heavy), {b: per[b] for b in sorted(set(heavy) | want_heavy)})
    # ---- buckets: empty ones in bulk, occupied ones one by one
    bucket = got["bucket"]
    in_range(case, "bucket", bucket, lambda ix: where(case, ix[0]))
    occ = sorted(ref.occupied)
    empty = np.ones(len(bucket), dtype=bool)
    empty[occ] = False
    w = 2 if case.g2 else 1
    zz = zero_mod_q(bucket[:, 2 * w:3 * w]).all(axis=-1)
    bad = np.flatnonzero(empty & ~zz)
    if bad.size:
        fail(case, "bucket (k_msm_bucket_finalize / k_msm_heavy)", "%s, which has no entries" % where(case, bad[0]), exp, bucket[bad[0]], 0)
    for b in occ:
        if not exp.matches(bucket[b], ref.bucket[b]):
            stage = "bucket (k_msm_heavy, %d pieces)" % per[b] if b in want_heavy else "bucket (k_msm_bucket_finalize, %d pieces)" % per[b]
            fail(case, stage, where(case, b), exp, bucket[b], ref.bucket[b])
    # ---- row and column sums, the weighted sum, the result
    H, L = case.tail.H, case.tail.L
    in_range(case, "partial_a", got["partial_a"], lambda ix: "element %d" % ix[0])
    for i, e in enumerate(ref.partial_a):
        if not exp.matches(got["partial_a"][i], e):
            s, r = divmod(i, H + L)
            fail(case, "partial_a (k_msm_rowcol_sum)", "set %d, %s" % (s, "Row_hi, hi = %d" % r if r < H else "Col_lo, lo = %d" % (r - H)), exp, got["partial_a"][i], e)
    in_range(case, "partial_b", got["partial_b"], lambda ix: "set %d" % ix[0])
    for s, e in enumerate(ref.partial_b):
        if not exp.matches(got["partial_b"][s], e):
            fail(case, "partial_b (k_msm_weighted_sum)", "set %d, sum_b (b + 1) B_b" % s, exp, got["partial_b"][s], e)
    res = got["result"]
    assert (np.array(F.limbs_to_ints(res), dtype=object) < FQ).all(), "%s: stage result: a coordinate is not canonical" % name
    if not exp.matches(res, ref.result):
        fail(case, "result (MsmWork::finish)", "sum_s 2^(c s) R_s", exp, res, ref.result)
    return got, info


def check_refusals(zk, oracle, monkeypatch, emulated):
    """null pointers, capacities, a second MSM with other buckets, offset / pos outside the borrowed sort, plog > 7: ZK_ERR_ARG each, and a
    good call behind every refusal still gives the right answer"""
    name = "borrowed_small"
    case = cases.CASES[name]
    make_bases(oracle, case)
    for k in ("ZK_MSM_QUAD", "ZK_MSM_QUAD_ACC", "ZK_ACC_PAIRS", "ZK_ROWCOL_SEG", "ZK_SEG_MIN", "ZK_SEG_MAX", "ZK_SORT_PER_GROUP"):
        monkeypatch.delenv(k, raising=False)
    m = case.first
    scal = F.fr_to_mont(m.scalars)
    first, keep = zk.msm_stage_in(case.bases[0], scal, n_src=m.n_sort, pos=m.pos, shift_payload=True)
    own, keep2 = zk.msm_stage_in(case.bases[0], scal[:m.n])
    small, keep3 = zk.msm_stage_in(case.bases[0][:4], scal[:4])
    c, W, nbt = case.c_used, case.shape.W, case.shape.nb
    bufs = dict(table=np.zeros((case.shape.rows * m.n, 2, 4), dtype=np.uint64), pieces=np.zeros((m.n_sort * W // 4 + nbt + 1, 4, 4), dtype=np.uint64),
                bucket=np.zeros((nbt, 4, 4), dtype=np.uint64), partial_a=np.zeros((case.tail.L + case.tail.H, 4, 4), dtype=np.uint64),
                partial_b=np.zeros((1, 4, 4), dtype=np.uint64), result=np.zeros((1, 2, 4), dtype=np.uint64), pieces2=np.zeros((m.n_sort * W // 4 + nbt + 1, 4, 4), dtype=np.uint64),
                off=np.zeros(nbt + 1, dtype=np.uint32), sorted=np.zeros(m.n_sort * W, dtype=np.uint32), heavy_list=np.zeros(nbt, dtype=np.uint32),
                off2=np.zeros(nbt + 1, dtype=np.uint32), sorted2=np.zeros(m.n_sort * W, dtype=np.uint32))
    u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

    def probe(a=first, b=None, c_=c, plog=0, null=(), caps=None, device=0):
        out = zk.ZkMsmStageOut()
        for k, arr in bufs.items():
            setattr(out, k, None if k in null else arr.ctypes.data_as(u64 if arr.dtype == np.uint64 else u32))
            cap = "heavy_cap" if k == "heavy_list" else k + "_cap"
            setattr(out, cap, (caps or {}).get(cap, arr.size))
        rc = zk._lib.zk_msm_stage_probe(0, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, 0, C.c_uint32(c_), C.c_uint32(plog),
                                        0, device, C.byref(out) if "out" not in null else None)
        return rc, out

    def good():
        for arr in bufs.values():
            arr[...] = 0
        rc, out = probe()
        assert rc == 0, zk._lib.zk_last_error()
        info = dict(zip(zk.STAGE_INFO, (int(v) for v in out.info)))
        exp = Expected(oracle, False, [Reference(case).result])
        assert exp.matches(bufs["result"][0], Reference(case).result), "%s: the result of a good call behind a refusal differs" % name
        return info

    def refused(what, **kw):
        for arr in bufs.values():
            arr[...] = 0
        rc, _ = probe(**kw)
        assert rc == ZK_ERR_ARG, "%s: answered %d, not ZK_ERR_ARG" % (what, rc)
        assert all(not arr.any() for arr in bufs.values()), "%s: refused, but an output was written" % what
        good()

    good()
    refused("first = NULL", a=None)
    refused("out = NULL", null=("out",))
    for k in ("table", "pieces", "bucket", "partial_a", "partial_b", "result", "off", "sorted", "heavy_list"):
        refused(k + " = NULL", null=(k,))
    for k in ("off2", "sorted2", "pieces2"):
        refused(k + " = NULL with a second MSM", b=own, null=(k,))
    need = dict(table_cap=case.shape.rows * m.n * 8, off_cap=nbt + 1, sorted_cap=m.n_sort * W, heavy_cap=nbt, bucket_cap=nbt * 16,
                partial_a_cap=(case.tail.L + case.tail.H) * 16, partial_b_cap=16, result_cap=8)
    for k, v in need.items():
        refused("%s one short" % k, caps={k: v - 1})
    refused("pieces_cap below the bucket count", caps={"pieces_cap": nbt * 16})
    refused("off2_cap one short", b=own, caps={"off2_cap": nbt})
    refused("plog = 8", plog=8)
    bad, _ = zk.msm_stage_in(case.bases[0], scal, n_src=m.n_sort, offset=m.n_sort - m.n + 1, shift_payload=True)
    refused("offset + n beyond n_src", a=bad)
    bad, _ = zk.msm_stage_in(case.bases[0], scal, n_src=m.n - 1, shift_payload=True)
    refused("more bases than sorted scalars", a=bad)
    pos = np.array(m.pos, dtype=np.uint32)
    pos[5] = m.n
    bad, keep4 = zk.msm_stage_in(case.bases[0], scal, n_src=m.n_sort, pos=pos, shift_payload=True)
    refused("pos names a base past n", a=bad)
    bad, _ = zk.msm_stage_in(case.bases[0], scal, n_src=m.n_sort, offset=3)
    refused("a second MSM with a borrowed sort", b=bad)
    for arr in bufs.values():
        arr[...] = 0
    assert probe(c_=0, b=small)[0] == ZK_ERR_ARG, "a second MSM whose buckets differ (c = 0: 4 scalars pick another width than 24) was not refused"
    assert b"other buckets" in zk._lib.zk_last_error() and all(not arr.any() for arr in bufs.values())
    good()
    del keep, keep2, keep3, keep4
