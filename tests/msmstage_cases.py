"""Inputs for the stage probe (zk_msm_stage_probe): the shapes of ethsnarks_amd/csrc/msm.hpp and msm_impl.hpp behind the bucket sort --
MsmShape::set, ChunkRule::len (helpers.ChunkRule), msm_piece_range, lo_bits / hi_bits and the seg_row / seg_col / row_groups / E arithmetic of
the bucket-reduction tail -- restated with Python integers, and cases that each ASSERT, from the restatement alone, that they reach the
shape they are named for, so that a later change of a constant cannot quietly turn one of them into an easy case (the convention of
msmsort_cases.py).  msmstage_checks.py runs them; nothing here touches a library.

Every base is a known multiple k G of the generator (k = 0: the affine infinity), so every value a stage leaves is e G for an integer e
mod r.  A scalar d 2^(c w) with 1 <= d <= 2^(c-1) has ONE digit, d in window w: one entry in bucket d - 1 of plane w mod 2^plog, reading
table row w >> plog.  The directed layouts are made of such scalars; their bucket contents are exact by construction.

The chunk length depends on the machine (ChunkRule.slots): an assertion that depends on it is made on import for the emulation build's
slots AND for a 256-CU device, and again at run time for the slots the probe's info block reports (Case.reaches)."""
from ethsnarks_amd import fields as F
from helpers import ChunkRule, rand_scalars
import msmsort_cases as sc

FR = F.FR
MSM_HEAVY, MSM_TREE, MSM_HEAVY_GRID = 64, 256, 256                        # msm.hpp
SEG_MIN, SEG_MIN_SMALL, SEG_MAX = 32, 8, 48
ABSENT = 0xffffffff
PIN8 = {"ZK_SEG_MAX": "8"}          # seg_min = seg_max = 8: ChunkRule.len gives 8 whatever the slots (asserted below)


def waves(g2, pairs):
    """Curve::WAVES_PER_SIMD / WAVES_PER_SIMD_PAIRS (bn254.hpp)"""
    return 2 if g2 else (3 if pairs else 4)


def machine_threads(emulated, waves_per_simd, cus=256):
    """msm_machine_threads"""
    return 32 * waves_per_simd if emulated else cus * 4 * waves_per_simd * 64


class Shape:
    """MsmShape::set + set_slots for n scalars sorted at window width c (batch 1), under the environment switches of `env`"""

    def __init__(self, n, c, plog, g2, env, tail_lanes=0):
        self.c, self.plog, self.W, self.nb = c, plog, sc.windows(c), 1 << (c - 1)
        self.sets = 1 << plog
        self.rows = (self.W + self.sets - 1) >> plog
        self.lo_bits, self.hi_bits = c // 2, (c - 1) - c // 2
        total = n * self.W
        self.quad = 4 if total <= 1 << 21 else 1
        self.quad_acc = 4 if total <= 1 << 17 else 1
        if "ZK_MSM_QUAD" in env:
            self.quad = 4 if int(env["ZK_MSM_QUAD"]) else 1
        if "ZK_MSM_QUAD_ACC" in env:
            self.quad_acc = 4 if int(env["ZK_MSM_QUAD_ACC"]) else 1
        self.acc_pairs = int(int(env["ZK_ACC_PAIRS"]) != 0 if "ZK_ACC_PAIRS" in env else total >= 3 << 21)
        self.rowcol_seg = 16
        v = int(env.get("ZK_ROWCOL_SEG", "0"))
        if 1 <= v <= 256 and not v & (v - 1):
            self.rowcol_seg = v
        self.seg_min, self.seg_max = (SEG_MIN_SMALL if total <= 1 << 23 else SEG_MIN), SEG_MAX
        if int(env.get("ZK_SEG_MIN", "0")) >= 4:
            self.seg_min = int(env["ZK_SEG_MIN"])
        if int(env.get("ZK_SEG_MAX", "0")) >= 4:
            self.seg_max = int(env["ZK_SEG_MAX"])
        self.seg_max = max(self.seg_max, self.seg_min)
        self.pairs_kernel = bool(self.acc_pairs) and not g2                # only G1 has k_msm_accumulate<C, 2>
        self.acc_form = 4 if self.quad_acc == 4 else (2 if self.pairs_kernel else 1)
        self.waves = waves(g2, self.pairs_kernel)
        self.tail_lanes = tail_lanes if tail_lanes in (1, 4) else self.quad

    def slots(self, emulated, cus=256):
        return max(machine_threads(emulated, self.waves, cus) // self.quad_acc, 1)

    def rule(self, slots):
        return ChunkRule(slots, self.seg_min, self.seg_max)

    def info(self):
        return {k: getattr(self, k) for k in ("c", "W", "nb", "plog", "sets", "lo_bits", "hi_bits", "quad", "quad_acc", "acc_pairs", "acc_form",
                                              "rowcol_seg", "seg_min", "seg_max", "tail_lanes", "rows")}


def piece_range(off, rule, b):
    """msm_piece_range: the chunk pieces [s0, s1) of bucket b (empty: 0, 0)"""
    e0, e1, seg = int(off[b]), int(off[b + 1]), rule.len(int(off[-1]))
    return (e0 // seg + b, (e1 - 1) // seg + b + 1) if e1 > e0 else (0, 0)


class Tail:
    """launch_reduce / k_msm_rowcol_sum / k_msm_weighted_sum: the shape of the row / column sums and of the weighted sum"""

    def __init__(self, c, lanes, rowcol_seg):
        self.L, self.H = 1 << (c // 2), 1 << ((c - 1) - c // 2)
        T = MSM_TREE // lanes
        want = T if lanes == 4 else rowcol_seg
        self.seg_row, self.seg_col = min(want, self.L), min(want, self.H)
        self.per_row, self.per_col = T // self.seg_row, T // self.seg_col          # lines per workgroup
        self.row_groups, self.col_groups = -(-self.H // self.per_row), -(-self.L // self.per_col)
        TH = T // 2
        self.W_row, self.W_col = min(self.H, TH), min(self.L, TH)                  # k_msm_weighted_sum: threads that hold elements, per half
        self.E_row, self.E_col = self.H // self.W_row, self.L // self.W_col        # ... and elements per thread


def single(d, w, c):
    """the scalar whose only digit is d (1 .. 2^(c-1)), in window w"""
    assert 1 <= d <= 1 << (c - 1) and w < sc.windows(c) and (d << (c * w)) < FR
    v = d << (c * w)
    assert [x for x in sc.signed_digits(v, c) if x] == [d] and sc.signed_digits(v, c)[w] == d
    return v


def base_multipliers(n, seed, distinct=100):
    """n base multipliers k_i over `distinct` values (seeded, non-zero), tiled"""
    ks = rand_scalars(min(n, distinct), seed)
    return [ks[i % len(ks)] or 1 for i in range(n)]


class Msm:
    """one multi-exponentiation of a case.  ks: the base multipliers (0 = affine infinity); scalars: the SORTED scalars (its own n, or the
    n_src of a borrowed sort); borrowed sort: offset / pos / shift as MsmWork::view_for and use_shift_payload take them"""

    def __init__(self, ks, scalars, borrowed=False, offset=0, pos=None, shift=False):
        self.ks, self.scalars, self.borrowed, self.offset, self.pos, self.shift = list(ks), list(scalars), borrowed, offset, pos, shift
        self.n, self.n_sort = len(self.ks), len(self.scalars)
        assert borrowed or (self.n == self.n_sort and pos is None and not offset and not shift)
        assert all(0 <= s < FR for s in self.scalars) and all(0 <= k < FR for k in self.ks)
        if borrowed:
            assert self.n <= self.n_sort and (pos is not None or offset + self.n <= self.n_sort)
            assert pos is None or (len(pos) == self.n_sort and all(p == ABSENT or p < self.n for p in pos))

    def base_of(self, i):
        """own base index of sorted scalar i, or None when this MSM has none for it (entry_index)"""
        if not self.borrowed:
            return i
        k = self.pos[i] if self.pos is not None else i - self.offset
        return k if 0 <= k < self.n else None


class Case:
    def __init__(self, name, g2, c, first, second=None, plog=0, tail_lanes=0, env=None, reaches=None, emul_only=False):
        self.name, self.g2, self.c, self.first, self.second, self.plog, self.tail_lanes = name, g2, c, first, second, plog, tail_lanes
        self.env, self._reaches, self.emul_only = dict(env or {}), reaches, emul_only
        self.sorts = [sc.Case(name, c, [m.scalars], plog=plog, shift=m.shift) for m in self.msms()]
        self.c_used = self.sorts[0].c_used
        self.shapes = [Shape(m.n_sort, s.c_used, plog, g2, self.env, tail_lanes) for m, s in zip(self.msms(), self.sorts)]
        self.shape = self.shapes[0]
        self.tail = Tail(self.c_used, self.shape.tail_lanes, self.shape.rowcol_seg)
        self.counts = [self._counts(s) for s in self.sorts]
        for emulated in (True, False) if not emul_only else (True,):
            self.reaches([sh.slots(emulated) for sh in self.shapes], emulated)

    def msms(self):
        return [self.first] + ([self.second] if self.second else [])

    @staticmethod
    def _counts(sort_case):
        """entries per bucket, from the scalars alone"""
        cnt, mask = [0] * sort_case.nb_total, (1 << sort_case.plog) - 1
        for s in sort_case.scalars[0]:
            for w, d in enumerate(sc.signed_digits(s, sort_case.c_used)):
                if d:
                    cnt[(w & mask) * sort_case.nbp + abs(d) - 1] += 1
        return cnt

    def offsets(self, side=0):
        off = [0]
        for v in self.counts[side]:
            off.append(off[-1] + v)
        return off

    def rules(self, slots):
        return [sh.rule(s) for sh, s in zip(self.shapes, slots)]

    def pieces_per_bucket(self, slots):
        """chunk pieces of every bucket, summed over the MSMs of the case (what k_msm_bucket_finalize compares with MSM_HEAVY)"""
        tot = [0] * len(self.counts[0])
        for side, rule in enumerate(self.rules(slots)):
            off = self.offsets(side)
            for b in range(len(tot)):
                s0, s1 = piece_range(off, rule, b)
                tot[b] += s1 - s0
        return tot

    def heavy_set(self, slots):
        return {b for b, p in enumerate(self.pieces_per_bucket(slots)) if p > MSM_HEAVY}

    def reaches(self, slots, emulated):
        """assert what the case is named for, for these slot counts (one per MSM)"""
        if self._reaches:
            self._reaches(self, slots, emulated)


# ---- layouts made of single-digit scalars
def layout(c, counts, seed, plane=0, plog=0):
    """scalars whose entries fill bucket b of `plane` with counts[b] entries (windows plane, plane + 2^plog, ... in turn: several table
    rows), and as many base multipliers"""
    S, sca = 1 << plog, []
    wins = [w for w in range(plane, sc.windows(c) - 1, S)][:3]
    for b, m in sorted(counts.items()):
        sca += [single(b + 1, wins[j % len(wins)], c) for j in range(m)]
    return base_multipliers(len(sca), seed), sca


def chunks_of(off, seg):
    """[(begin, end, buckets touched)] of every chunk of the entry list"""
    total, out = off[-1], []
    bucket_of = [b for b in range(len(off) - 1) for _ in range(off[b + 1] - off[b])]
    for begin in range(0, total, seg):
        end = min(begin + seg, total)
        out.append((begin, end, sorted(set(bucket_of[begin:end]))))
    return out


BOUNDARY_COUNTS = {0: 8, 1: 1, 2: 7, 3: 9, 4: 17, 7: 1, 8: 1, 10: 2, 11: 3, 12: 5}     # buckets of 1, 7, 8, 9 and 17 entries; 5, 6 and 9 stay empty


def _boundaries(case, slots, emulated):
    off, rule = case.offsets(), case.rules(slots)[0]
    seg = rule.len(off[-1])
    assert seg == 8 == rule.seg_min and rule.seg_min * rule.slots >= off[-1], "the branch seg = seg_min = 8, the one a device takes below about 2 M entries"
    ch = chunks_of(off, seg)
    starts = {off[b] for b in range(len(off) - 1) if off[b + 1] > off[b]}
    assert any(b and b in starts for b, _, _ in ch), "a chunk starts exactly on a bucket boundary"
    assert any(e in starts or e == off[-1] for _, e, _ in ch[:-1]), "a chunk ends exactly on one (its last flush writes a whole piece)"
    assert any(len(bs) >= 4 and any(y - x > 1 for x, y in zip(bs, bs[1:])) for _, _, bs in ch), "a chunk crosses three boundaries, one behind empty buckets"
    assert ch[-1][1] - ch[-1][0] < seg, "the last chunk is short"
    assert sorted(set(case.counts[0]) - {0}) == [1, 2, 3, 5, 7, 8, 9, 17]
    assert not case.heavy_set(slots)


def _holds(pred):
    def check(case, slots, emulated):
        assert pred(case, slots), case.name
    return check


def _branch(multi_round=None, seg=None):
    def check(case, slots, emulated):
        off, rule = case.offsets(), case.rules(slots)[0]
        if emulated and multi_round is not None:
            assert (rule.seg_min * rule.slots < off[-1]) == multi_round
        if emulated and seg is not None:
            assert rule.len(off[-1]) == seg, (case.name, rule.len(off[-1]), seg)
    return check


def _pieces_of(want, side_counts=None):
    """want: {bucket: pieces summed over the MSMs}; heavy exactly where that exceeds MSM_HEAVY.  side_counts: {bucket: (pieces first, second)}"""
    def check(case, slots, emulated):
        rules = case.rules(slots)
        assert all(r.len(o[-1]) == 8 for r, o in zip(rules, (case.offsets(0), case.offsets(len(rules) - 1))))
        per = case.pieces_per_bucket(slots)
        for b, p in want.items():
            assert per[b] == p, (case.name, b, per[b], p)
        assert case.heavy_set(slots) == {b for b, p in want.items() if p > MSM_HEAVY}
        for b, (p1, p2) in (side_counts or {}).items():
            for side, p in ((0, p1), (1, p2)):
                s0, s1 = piece_range(case.offsets(side), rules[side], b)
                assert s1 - s0 == p, (case.name, b, side, s1 - s0, p)
    return check


# ---- the row / column and weighted sums: what each width reaches, per lanes of the tail (stated here, asserted against Tail)
#   (c, lanes): (relation of the bucket matrix, E of the row half, E of the column half)
TAIL_WIDTHS = (2, 3, 4, 9, 12, 13, 16, 17, 20)
TAIL_G2_WIDTHS = (2, 13, 17)
TAIL_REACHES = {
    (2, 1): ("H=1", 1, 1), (2, 4): ("H=1", 1, 1),
    (3, 1): ("L=H", 1, 1), (3, 4): ("L=H", 1, 1),
    (4, 1): ("L=2H", 1, 1), (4, 4): ("L=2H", 1, 1),
    (9, 1): ("L=H", 1, 1), (9, 4): ("L=H", 1, 1),
    (12, 1): ("L=2H", 1, 1), (12, 4): ("L=2H", 1, 2),                     # E > 1 in the column half only
    (13, 1): ("L=H", 1, 1), (13, 4): ("L=H", 2, 2),                       # ... in both
    (16, 1): ("L=2H", 1, 2), (16, 4): ("L=2H", 4, 8),
    (17, 1): ("L=H", 2, 2), (17, 4): ("L=H", 8, 8),
    (20, 1): ("L=2H", 4, 8), (20, 4): ("L=2H", 16, 32),
}


def _tail_reaches(case, slots, emulated):
    t, lanes = case.tail, case.shape.tail_lanes
    rel, e_row, e_col = TAIL_REACHES[(case.c_used, lanes)]
    assert (t.E_row, t.E_col) == (e_row, e_col), (case.name, t.E_row, t.E_col)
    assert {"H=1": t.H == 1, "L=H": t.L == t.H > 1, "L=2H": t.L == 2 * t.H}[rel], case.name
    if lanes == 4:
        assert (t.seg_row, t.seg_col) == (min(64, t.L), min(64, t.H))    # clamped by L / H up to c = 12


def corners(c):
    nb, L = 1 << (c - 1), 1 << (c // 2)
    return sorted({b for b in (0, L - 1, L, nb - L, nb - 1) if 0 <= b < nb})


def corner_plog(c):
    return 3 if c <= 17 else 1                                            # (sets x buckets stay within the sort's 2^20)


def corner_cases(c, g2, lanes):
    """one occupied bucket at each corner b = 0, L - 1, L, nb - L, nb - 1 in turn: every corner alone in a bucket SET of its own (the
    planes of a frugal table are reduced side by side, each by its own workgroups); the remaining sets stay empty"""
    plog, cs, out = corner_plog(c), corners(c), []
    S = 1 << plog
    for part in range(0, len(cs), S):
        sca = [single(b + 1, j, c) for j, b in enumerate(cs[part:part + S])]

        def reach(case, slots, emulated, want=cs[part:part + S]):
            _tail_reaches(case, slots, emulated)
            for j, b in enumerate(want):
                assert [i for i, v in enumerate(case.counts[0][j * case.shape.nb:(j + 1) * case.shape.nb]) if v] == [b]
            assert sum(case.counts[0]) == len(want)
        out.append(Case("corners%d_c%d_%s_q%d" % (part // S, c, "g2" if g2 else "g1", lanes), g2, c, Msm(base_multipliers(len(sca), 300 + c), sca),
                        plog=plog, tail_lanes=lanes, reaches=reach))
    return out


def equal_case(c, g2, lanes):
    """the same point in every bucket: scalars 1 .. nb over one repeated base; every addition of every tree and scan meets equal operands"""
    nb = 1 << (c - 1)
    k = rand_scalars(1, 400 + c)[0]

    def reach(case, slots, emulated):
        _tail_reaches(case, slots, emulated)
        assert case.counts[0] == [1] * nb and len(set(case.first.ks)) == 1
    return Case("equal_c%d_%s_q%d" % (c, "g2" if g2 else "g1", lanes), g2, c, Msm([k] * nb, list(range(1, nb + 1))), tail_lanes=lanes, reaches=reach)


def alternating_case(c, g2, lanes, along_rows):
    """P and -P alternating along every row (lo parity) or along every column (hi parity): whole rows resp. columns sum to infinity"""
    nb, L = 1 << (c - 1), 1 << (c // 2)
    k = rand_scalars(1, 500 + c)[0]
    sign = lambda b: (b % L if along_rows else b // L) & 1
    ks = [(FR - k) if sign(b) else k for b in range(nb)]

    def reach(case, slots, emulated):
        _tail_reaches(case, slots, emulated)
        assert case.counts[0] == [1] * nb
        H = nb // L
        if along_rows:
            assert all(sum(ks[h * L + l] for l in range(L)) % FR == 0 for h in range(H))
        else:
            assert H >= 2 and all(sum(ks[h * L + l] for h in range(H)) % FR == 0 for l in range(L))
    return Case("alt_%s_c%d_%s_q%d" % ("rows" if along_rows else "cols", c, "g2" if g2 else "g1", lanes), g2, c, Msm(ks, list(range(1, nb + 1))),
                tail_lanes=lanes, reaches=reach)


def random_case(name, c, g2, n, seed, reaches=None, infinity_at=None, **kw):
    ks = base_multipliers(n, seed)
    if infinity_at is not None:
        ks[infinity_at] = 0
    return Case(name, g2, c, Msm(ks, sc._rand(n, seed, c)), reaches=reaches, **kw)


def _build():
    cases = {}

    def add(case):
        assert case.name not in cases, case.name
        cases[case.name] = case
        return case

    # ---- the table: plog = 0, 1, 2 at c = 5 and c = 16, 65 bases (one full wave and one lane), one of them the affine infinity
    for c in (5, 16):
        for plog in (0, 1, 2):
            def reach(case, slots, emulated, c=c, plog=plog):
                s = case.shape
                assert case.first.n == 65 and case.first.ks.count(0) == 1 and s.rows == -(-sc.windows(c) >> plog) and s.sets == 1 << plog
                assert (s.rows * s.sets > s.W) == (c == 5 and plog > 0)       # (c = 5: W = 51, the last row serves fewer planes)
            add(random_case("table_c%d_plog%d" % (c, plog), c, False, 65, 20 + c + plog, plog=plog, infinity_at=17, reaches=reach))
    add(random_case("table_n1", 5, False, 1, 31))
    add(random_case("table_g2_c5_plog1", 5, True, 65, 32, plog=1, infinity_at=64))
    # the frugal planes with four sets: the set stride of partial_a and the host fold of finish()
    add(random_case("planes4_c5", 5, False, 300, 33, plog=2, tail_lanes=1,
                    reaches=_holds(lambda case, slots: (case.shape.sets, case.shape.rows, case.shape.W) == (4, 13, 51))))

    # ---- accumulation: chunks against bucket boundaries, every lane form
    for g2, forms in ((False, (1, 2, 4)), (True, (1, 4))):
        for q in forms:
            env = {"ZK_MSM_QUAD_ACC": "1" if q == 4 else "0", "ZK_ACC_PAIRS": "1" if q == 2 else "0"}

            def reach(case, slots, emulated, q=q):
                assert case.shape.acc_form == q
                _boundaries(case, slots, emulated)
            ks, sca = layout(5, BOUNDARY_COUNTS, 40 + q)
            add(Case("boundaries_%s_q%d" % ("g2" if g2 else "g1", q), g2, 5, Msm(ks, sca), env=env, reaches=reach))
    # the multi-round branch of ChunkRule::len (the emulation build's slots), and ZK_SEG_MIN = 4
    add(random_case("rounds_1500", 7, False, 40, 51, emul_only=True, reaches=_branch(multi_round=True)))
    add(random_case("rounds_5000", 7, False, 140, 52, emul_only=True, reaches=_branch(multi_round=True)))
    add(random_case("rounds_5000_q1", 7, False, 140, 53, emul_only=True, env={"ZK_MSM_QUAD_ACC": "0"}, reaches=_branch(multi_round=True)))
    add(random_case("seg_min_4", 7, False, 40, 54, env={"ZK_SEG_MIN": "4", "ZK_SEG_MAX": "4"},
                    reaches=_holds(lambda case, slots: case.rules(slots)[0].len(case.offsets()[-1]) == 4)))
    # a borrowed sort: (row << kbits) | i entries or row * n_src + i, an offset without pos, and a pos that leaves a third of the scalars out
    n_src, n_own = 150, 90
    for g2 in (False, True):
        for shift in (True, False):
            src = sc._rand(n_src, 60 + shift, 7)

            def reach(case, slots, emulated, shift=shift):
                assert (case.sorts[0].kbits != 0) == shift and case.first.borrowed
            tag = "%s_%s" % ("g2" if g2 else "g1", "kbits" if shift else "div")
            add(Case("borrowed_offset_" + tag, g2, 7, Msm(base_multipliers(n_own, 61), src, borrowed=True, offset=37, shift=shift), reaches=reach))
            pos = [ABSENT if i % 3 == 0 or i == n_src - 1 else (7 * i) % n_own for i in range(n_src)]

            def reach_pos(case, slots, emulated, pos=pos, inner=reach):
                inner(case, slots, emulated)
                assert pos[0] == ABSENT and pos[-1] == ABSENT and n_src // 3 <= pos.count(ABSENT) <= n_src // 3 + 2
            if not g2 or shift:
                add(Case("borrowed_pos_" + tag, g2, 7, Msm(base_multipliers(n_own, 62), src, borrowed=True, pos=pos, shift=shift), reaches=reach_pos))

    # a small one for the probe's refusals (few buckets: a cheap call on the emulation build)
    pos = [ABSENT if i % 3 == 0 or i == 23 else (5 * i) % 16 for i in range(24)]
    add(Case("borrowed_small", False, 3, Msm(base_multipliers(16, 63), sc._rand(24, 64, 3), borrowed=True, pos=pos, shift=True),
             reaches=_holds(lambda case, slots: case.sorts[0].kbits == 5 and sc.pick_c(24) != sc.pick_c(4))))

    # ---- bucket sums and the heavy list: exactly 64 pieces (light), 65 by alignment, 65 by count; both tail lane counts
    qacc0 = dict(PIN8, ZK_MSM_QUAD_ACC="0")
    for lanes in (1, 4):
        for g2 in (False, True):
            t = "%s_t%d" % ("g2" if g2 else "g1", lanes)
            ks, sca = layout(5, {0: 512, 3: 5}, 70)
            add(Case("heavy_64_exact_" + t, g2, 5, Msm(ks, sca), env=qacc0, tail_lanes=lanes, reaches=_pieces_of({0: 64, 3: 1})))
            if g2 and lanes == 1:
                continue
            ks, sca = layout(5, {0: 7, 1: 506, 9: 3}, 71)
            add(Case("heavy_65_aligned_" + t, g2, 5, Msm(ks, sca), env=qacc0, tail_lanes=lanes, reaches=_pieces_of({0: 1, 1: 65, 9: 1})))
            ks, sca = layout(5, {0: 513, 15: 2}, 72)
            add(Case("heavy_65_count_" + t, g2, 5, Msm(ks, sca), env=qacc0, tail_lanes=lanes, reaches=_pieces_of({0: 65, 15: 1})))
        # the merged tail: 40 + 40 (heavy only by the sum), 64 + 0 (light), 0 + 65, 130 + 3 (lane stride 128 straddles the seam)
        for g2 in (False, True):
            if g2 and lanes == 1:
                continue
            k1, s1 = layout(7, {3: 320, 10: 512, 40: 1040}, 73)
            k2, s2 = layout(7, {3: 320, 20: 520, 40: 24}, 74)
            add(Case("merged_%s_t%d" % ("g2" if g2 else "g1", lanes), g2, 7, Msm(k1, s1), second=Msm(k2, s2), env=qacc0, tail_lanes=lanes,
                     reaches=_pieces_of({3: 80, 10: 64, 20: 65, 40: 133}, {3: (40, 40), 10: (64, 0), 20: (0, 65), 40: (130, 3)})))

    # ---- row / column sums and the weighted sum, at every width that changes their shape
    for g2, widths in ((False, TAIL_WIDTHS), (True, TAIL_G2_WIDTHS)):
        for c in widths:
            for lanes in (1, 4):
                for case in corner_cases(c, g2, lanes):
                    add(case)
                add(random_case("sparse_c%d_%s_q%d" % (c, "g2" if g2 else "g1", lanes), c, g2, 120, 80 + c, tail_lanes=lanes, reaches=_tail_reaches))
                if c <= 13:
                    add(equal_case(c, g2, lanes))
                    add(alternating_case(c, g2, lanes, True))
                    if c >= 3:
                        add(alternating_case(c, g2, lanes, False))
    # threads per row / column: 1 (per > lines: one workgroup holds more lines than there are), 16, 256 (clamped by L and H)
    for seg in (1, 16, 256):
        def reach(case, slots, emulated, seg=seg):
            t = case.tail
            assert case.shape.rowcol_seg == seg and (t.seg_row, t.seg_col) == (min(seg, 16), min(seg, 16)) and (t.L, t.H) == (16, 16)
            assert (t.per_row > t.H) == (seg == 1) and t.row_groups == t.col_groups == {1: 1, 16: 1, 256: 1}[seg]
        add(random_case("rowcol_seg%d_c9" % seg, 9, False, 300, 90 + seg, tail_lanes=1, env={"ZK_ROWCOL_SEG": str(seg)}, reaches=reach))
    add(random_case("rowcol_seg16_c13", 13, False, 300, 95, tail_lanes=1,
                    reaches=_holds(lambda case, slots: (case.tail.row_groups, case.tail.col_groups, case.tail.per_row) == (4, 4, 16))))
    return cases


CASES = _build()
TABLE_CASES = tuple(k for k in CASES if k.startswith(("table_", "planes4")))
ACC_CASES = tuple(k for k in CASES if k.startswith(("boundaries_", "rounds_", "seg_min", "borrowed_")))
HEAVY_CASES = tuple(k for k in CASES if k.startswith(("heavy_", "merged_")))
TAIL_CASES = tuple(k for k in CASES if k.startswith(("corners", "sparse_", "equal_", "alt_", "rowcol_")))
assert len(TABLE_CASES) + len(ACC_CASES) + len(HEAVY_CASES) + len(TAIL_CASES) == len(CASES)
DEVICE_CASES = tuple(k for k in CASES if not CASES[k].emul_only)
