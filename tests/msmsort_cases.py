"""Inputs for the bucket-sort probe (zk_msm_sort_probe): the window recoding and the sort shapes of ethsnarks_amd/csrc/msm.hpp and
msm_impl.hpp restated with Python integers, scalar families built per window width c for the edges of the signed-digit recoding, and
cases that each ASSERT, from the restatement alone, that they reach the sort shape they are named for -- so that a later change of a
constant cannot quietly turn one of them into an easy case.  msmsort_checks.py runs them; nothing here touches a library.

  msm_digit        digit = window bits + carry; above 2^(c-1) it becomes digit - 2^c with a carry into the next window
  bucket id        ((proof << plog) | (w mod 2^plog)) * 2^(c-1) + |d| - 1
  payload          row * n + i, or (row << kbits) | i for the shared witness sort; row = w >> plog; the sign in bit 31
"""
import functools
import numpy as np
from ethsnarks_amd import fields as F
from helpers import rand_scalars

FR = F.FR
SORT_THREADS, SORT_MAX_CB, SORT_MAX_FB, SORT_STAGE, MSM_SEG_MIN = 256, 256, 4096, 7680, 32      # msm.hpp
WIDTHS = tuple(range(2, 21))


def windows(c):
    return 254 // c + 1


# ---- the shapes, restated
def pick_c(n, batch=1):
    """MsmShape::pick_c"""
    for c in range(17, 2, -1):
        entries = n * windows(c)
        floor_c = 2 * MSM_SEG_MIN - 1 if c >= 16 else MSM_SEG_MIN
        per_bucket = floor_c
        if batch > 1:
            per_bucket = max(min(32 * entries * batch // 1482910, 100), floor_c)
        if entries >= per_bucket << (c - 1):
            return c
    return 2


class SortShape:
    """SortShape::set / resize for n scalars (of all proofs) and nb buckets (of all bucket sets)"""

    def __init__(self, n, nb, W, env):
        self.per_group = 512
        while self.per_group > 32 and self.per_group * W > SORT_STAGE:
            self.per_group >>= 1
        v = env.get("ZK_SORT_PER_GROUP")
        if v is not None and int(v) >= 64:
            self.per_group = int(v)
        self.fine_bits = 0
        while (nb + (1 << self.fine_bits) - 1) >> self.fine_bits > SORT_MAX_CB:
            self.fine_bits += 1
        self.fb = 1 << self.fine_bits
        self.cb = (nb + self.fb - 1) >> self.fine_bits
        self.groups = max((n + self.per_group - 1) // self.per_group, 1)
        self.staged = self.per_group * W <= SORT_STAGE                  # MsmWork::enqueue_sort: k_sort_partition_staged, else k_sort_partition
        assert self.fb <= SORT_MAX_FB and self.cb <= SORT_MAX_CB


def shift_kbits(n, rows):
    """MsmWork::use_shift_payload"""
    k = 1
    while 1 << k < n:
        k += 1
    return k if rows << k < 1 << 31 else 0


# ---- the recoding, restated
def signed_digits(s, c):
    """the W signed digits of the canonical scalar s, lowest window first (msm_digit with its carry chain)"""
    nbp, full, out, carry = 1 << (c - 1), 1 << c, [], 0
    for w in range(windows(c)):
        d = ((s >> (w * c)) & (full - 1)) + carry
        carry = 0
        if d > nbp:
            d, carry = d - full, 1
        out.append(d)
    assert carry == 0 and sum(d << (w * c) for w, d in enumerate(out)) == s, "a scalar below r recodes without a carry out of the top window"
    return out


def carry_ins(s, c):
    """carry_ins(s, c)[w]: the carry that window w receives"""
    nbp, full, out, carry = 1 << (c - 1), 1 << c, [], 0
    for w in range(windows(c)):
        out.append(carry)
        carry = int(((s >> (w * c)) & (full - 1)) + carry > nbp)
    return out


def carry_into_top(s, c):
    return carry_ins(s, c)[-1] == 1


def full_carry_chain(c):
    """2^(c-1) + 1 in window 0 and 2^(c-1) in every window below the top one: each of them overflows only through the carry it receives,
    so the chain runs through all W windows and leaves +1 in the top one (the value is below 2^253 for c > 2, and 0.67 x 2^254 < r at c = 2)"""
    return 1 + sum(1 << (c - 1) << (c * w) for w in range(windows(c) - 1))


def all_windows(pattern, c):
    """every window equal to `pattern`, cut at the top window(s) so that the value stays below r"""
    W = windows(c)
    v = sum(pattern << (c * w) for w in range(W)) & ((1 << 256) - 1)
    while v >= FR:
        W -= 1
        v &= (1 << (c * W)) - 1
    return v


def largest_with_carry_into_top(c):
    """the largest scalar below r whose top window receives a carry.  The windows below the top one (k bits) carry out exactly when their
    value exceeds what positive digits alone can represent, which is monotone in that value: so it is r - 1 if r - 1 does, and otherwise
    the largest value with a smaller top part, whose low k bits are all ones (and do carry)."""
    k = (windows(c) - 1) * c
    for v in (FR - 1, (((FR - 1) >> k) << k) - 1):
        if carry_into_top(v, c):
            return v
    raise AssertionError("no scalar with a carry into the top window at c = %d" % c)


FIXED = (("0", 0), ("1", 1), ("2", 2), ("r-1", FR - 1), ("r-2", FR - 2), ("(r-1)/2", (FR - 1) // 2), ("(r+1)/2", (FR + 1) // 2), ("2^253", 1 << 253))


@functools.lru_cache(maxsize=None)
def edge_scalars(c):
    """[(label, canonical value)]: the recoding edges of window width c"""
    nbp, W = 1 << (c - 1), windows(c)
    out = list(FIXED)
    out += [("2^%d" % k, 1 << k) for k in range(254)]                   # one digit, in every window, at every bit offset of a limb
    out += [("2^%d-1" % k, (1 << k) - 1) for k in range(1, 254)]        # carry chains of every length
    out += [("all windows 2^(c-1)", all_windows(nbp, c)),               # no carry, the largest bucket
            ("all windows 2^(c-1)+1", all_windows(nbp + 1, c)),         # every digit negative, a carry into every window
            ("all windows 2^c-1", all_windows((1 << c) - 1, c)),        # digit -1, then zeros made by the carry
            ("carry chain through all windows", full_carry_chain(c)),
            ("largest with a carry into the top window", largest_with_carry_into_top(c))]
    assert all(0 <= v < FR for _, v in out)
    dig = {label: signed_digits(v, c) for label, v in out}
    # what the family is there for, asserted from the restatement
    a = dig["all windows 2^(c-1)"]
    assert a[0] == nbp and all(d in (nbp, 0) for d in a) and a.count(nbp) >= W - 2
    b = dig["all windows 2^(c-1)+1"]
    if c > 2:                                                            # (at c = 2 this is the next pattern: 2^(c-1) + 1 = 2^c - 1)
        assert b[0] == -(nbp - 1) and b.count(-(nbp - 2)) >= W - 4 and sum(carry_ins(all_windows(nbp + 1, c), c)) >= W - 3
    z = dig["all windows 2^c-1"]
    assert z[0] == -1 and z.count(0) >= W - 3 and sum(abs(d) for d in z) == 2, "digit -1, zeros made by the carry, and the carry's +1 at the end"
    assert carry_ins(full_carry_chain(c), c) == [0] + [1] * (W - 1) and all(dig["carry chain through all windows"])
    assert carry_into_top(out[-1][1], c) and dig[out[-1][0]][W - 1] != 0
    top = (W - 1) * c
    if top + c > 256:                                                    # the top window reaches past the scalar's last limb, and limb + 1 == 8 reads as 0
        assert top >> 5 == 7 and any(dig["2^%d" % k][W - 1] for k in range(top, 254))
    for lim in range(32, 254, 32):                                       # a window cut by a limb boundary: single digits on either side of the cut
        w = lim // c
        if w * c < lim:
            assert dig["2^%d" % (lim - 1)][w] == 1 << (lim - 1 - w * c) and dig["2^%d" % lim][w] == 1 << (lim - w * c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def family(c, filler=600):
    """the edge scalars of width c and `filler` seeded random ones, so that buckets hold several entries"""
    return tuple(v for _, v in edge_scalars(c)) + tuple(rand_scalars(filler, 1000 + c))


def label_of(c, value):
    return next((label for label, v in edge_scalars(c) if v == value), "random")


# ---- cases
class Case:
    """one probe call: `scalars` is a tuple of `batch` tuples of `stride` canonical ints, of which the first n of each are sorted"""

    def __init__(self, name, c, scalars, n=None, plog=0, shift=False, env=None, forms=("mont",), expect=None):
        self.name, self.c, self.plog, self.shift, self.env, self.forms = name, c, plog, shift, dict(env or {}), forms
        self.scalars = tuple(tuple(p) for p in scalars)
        self.batch, self.stride = len(self.scalars), len(self.scalars[0])
        assert all(len(p) == self.stride for p in self.scalars) and all(0 <= v < FR for p in self.scalars for v in p)
        self.n = self.stride if n is None else n
        self.c_used = min(max(c, 2), 20) if c else pick_c(self.n or 1, self.batch)
        self.W, self.nbp = windows(self.c_used), 1 << (self.c_used - 1)
        self.nb_total = (self.nbp * self.batch) << plog
        self.rows = (self.W + (1 << plog) - 1) >> plog
        self.shape = SortShape(self.n * self.batch or 1, self.nb_total, self.W, self.env)
        self.kbits = shift_kbits(self.n, self.rows) if shift else 0
        if expect:
            expect(self)

    def info(self):
        s = self.shape
        return dict(c=self.c_used, W=self.W, nb_total=self.nb_total, cb=s.cb, fb=s.fb, fine_bits=s.fine_bits, groups=s.groups,
                    per_group=s.per_group, sort_kbits=self.kbits, staged=int(s.staged))

    def sorted_scalars(self):
        return [p[:self.n] for p in self.scalars]


def straddles(case):
    """a pass-1 workgroup whose run of scalars crosses from one proof into the next"""
    pg, n, total = case.shape.per_group, case.n, case.n * case.batch
    return any(g * pg // n != (min((g + 1) * pg, total) - 1) // n for g in range(case.shape.groups))


def _expect(**want):
    def check(case):
        have = dict(case.info(), batch=case.batch, n=case.n)
        for k, v in want.items():
            assert have[k] == v, (case.name, k, have[k], v)
    return check


def _holds(pred):
    def check(case):
        assert pred(case), case.name
    return check


def _both(*fs):
    def check(case):
        for f in fs:
            f(case)
    return check


def _width(c, env=None, tag="width"):
    def check(case):
        s = case.shape
        assert s.fine_bits == max(0, c - 9) and s.cb == min(case.nbp, 256) and s.cb * s.fb == case.nb_total
        assert case.c_used == c and case.W == windows(c)
        if env is None:
            assert s.staged and s.groups >= 2, "the default per_group always fits the staged partition"
            assert c > 2 or (case.W, s.per_group) == (128, 32)
        if c >= 18:
            assert case.n * case.W * 4 < case.nb_total, "at least three buckets in four are empty"
    return Case("%s_c%d" % (tag, c), c, [family(c)], env=env, forms=("mont", "canon") if env is None else ("mont",), expect=check)


def _rand(n, seed, c, edges=40):
    """n scalars: seeded random ones with every edges-th edge scalar of width c mixed in"""
    sc = rand_scalars(n, seed)
    e = [v for _, v in edge_scalars(c)]
    for j, i in enumerate(range(0, n, 7)):
        sc[i] = e[(j * edges + seed) % len(e)]
    return sc


def _batch(k, n, stride, c, seed):
    """k proofs with DIFFERENT scalars each; the stride gap holds r - 1, whose digits would show if a kernel read it"""
    return [_rand(n, seed + 31 * p, c) + [FR - 1] * (stride - n) for p in range(k)]


def _build():
    cases = {}

    def add(case):
        assert case.name not in cases
        cases[case.name] = case

    for c in WIDTHS:
        add(_width(c))
    # scalar counts around a pass-1 workgroup
    for c, pg in ((7, 128), (13, 256)):
        for tag, n, groups in (("n0", 0, 1), ("n1", 1, 1), ("n_per_group", pg, 1), ("n_per_group_plus_1", pg + 1, 2), ("three_groups", 2 * pg + 57, 3)):
            add(Case("%s_c%d" % (tag, c), c, [_rand(n, 50 + n, c)], expect=_expect(n=n, per_group=pg, groups=groups, staged=1)))
    # batches whose workgroups cross from one proof into the next
    for k, fine_bits, cb in ((2, 3, 256), (3, 4, 192), (5, 5, 160)):
        add(Case("batch%d" % k, 11, _batch(k, 300, 307, 11, 7 * k), n=300,
                 expect=_both(_expect(batch=k, per_group=256, fine_bits=fine_bits, cb=cb, groups=(300 * k + 255) // 256),
                              _holds(straddles))))
    # a partly filled last coarse bin: 257 proofs of 2 buckets each are 514 buckets in 129 bins of 4
    def partial(case):
        s = case.shape
        assert s.cb * s.fb > case.nb_total and (s.cb - 1) * s.fb < case.nb_total and (s.cb, s.fb, case.nb_total) == (129, 4, 514)
    add(Case("partial_last_bin", 2, _batch(257, 3, 4, 2, 3), n=3, expect=_both(partial, _expect(per_group=32, groups=25))))
    # as many buckets as the sort holds: 256 coarse bins of 4096 fine buckets
    add(Case("max_buckets", 20, _batch(2, 40, 41, 20, 5), n=40, expect=_expect(nb_total=1 << 20, cb=SORT_MAX_CB, fb=SORT_MAX_FB, fine_bits=12)))
    # bucket planes, alone and with a batch; c = 12 has W = 22 windows, so with four planes the last table row serves only two of them
    add(Case("planes2", 12, [_rand(700, 61, 12)], plog=1, expect=_expect(nb_total=2 << 11, W=22)))
    add(Case("planes4_partial_row", 12, [_rand(700, 62, 12)], plog=2,
             expect=_both(_expect(nb_total=4 << 11, W=22), _holds(lambda case: case.rows * 4 > case.W and case.rows == 6))))
    add(Case("planes2_batch3", 9, _batch(3, 300, 301, 9, 63), n=300, plog=1,
             expect=_both(_expect(nb_total=6 << 8, W=29, batch=3), _holds(lambda case: case.rows * 2 > case.W and straddles(case)))))
    # the payload of the shared witness sort; kbits changes between n = 2^9 and 2^9 + 1
    add(Case("shift_n512", 10, [_rand(512, 71, 10)], shift=True, expect=_expect(sort_kbits=9)))
    add(Case("shift_n513", 10, [_rand(513, 72, 10)], shift=True, expect=_expect(sort_kbits=10)))
    add(Case("plain_n513", 10, [_rand(513, 72, 10)], expect=_expect(sort_kbits=0)))
    add(Case("shift_planes2_batch2", 10, _batch(2, 513, 520, 10, 73), n=513, plog=1, shift=True, expect=_expect(sort_kbits=10, batch=2)))
    add(Case("shift_n1", 10, [[FR - 1]], shift=True, expect=_expect(sort_kbits=1)))
    # the library's own choice of c
    add(Case("picked_width", 0, [_rand(2000, 81, 11)], expect=_expect(c=11)))
    add(Case("picked_width_batch3", 0, _batch(3, 700, 700, 11, 82), expect=_expect(c=pick_c(700, 3))))
    # ZK_SORT_PER_GROUP = 1024: W >= 13 windows each are more than the staged partition holds, the direct scatter runs
    for c in WIDTHS:
        add(_width(c, env={"ZK_SORT_PER_GROUP": "1024"}, tag="direct"))
        assert not cases["direct_c%d" % c].shape.staged and cases["direct_c%d" % c].shape.groups == 2
    # ZK_SORT_PER_GROUP = 64: many small workgroups (staged wherever 64 W <= SORT_STAGE, that is from c = 3 on)
    for c in (2, 3, 8, 13, 17, 20):
        add(_width(c, env={"ZK_SORT_PER_GROUP": "64"}, tag="small_groups"))
        s = cases["small_groups_c%d" % c].shape
        assert s.staged == (c >= 3) and s.groups >= 13 and s.per_group == 64
    # one value everywhere
    for c in (5, 13):
        one = rand_scalars(1, 90 + c)[0]
        add(Case("all_equal_c%d" % c, c, [[one] * 700], expect=_holds(lambda case: sum(1 for d in signed_digits(case.scalars[0][0], case.c_used) if d) >= case.W * 3 // 4)))
        add(Case("all_in_one_bucket_c%d" % c, c, [[all_windows(1 << (c - 1), c)] * 700]))
    add(Case("all_zero", 13, [[0] * 500]))
    return cases


CASES = _build()
WIDTH_CASES = tuple("width_c%d" % c for c in WIDTHS)
DIRECT_CASES = tuple("direct_c%d" % c for c in WIDTHS)
SHAPE_CASES = tuple(k for k in CASES if k not in WIDTH_CASES and k not in DIRECT_CASES)


# ---- the end-to-end multi-exponentiations
MSM_G1_WIDTHS, MSM_G2_WIDTHS = WIDTHS, (2, 9, 13, 17, 20)
MSM_DISTINCT = 100


def msm_scalars(c):
    """the edge scalars of width c (over MSM_DISTINCT tiled bases), then 3, 3 for a base and its negation and 4, 4 for a base twice"""
    return [v for _, v in edge_scalars(c)] + [3, 3, 4, 4]
