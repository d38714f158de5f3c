"""The compiled program of a wide witness plan (zk_wplan_probe_program), decoded from the record format documented at the top of
csrc/wplan_wide.hpp, checked against the contract k_witness_wide relies on, and run over Python integers.

The contract: inside one pass (between two barriers) no lane reads an LDS slot or a witness-row variable that another lane of the group
writes in that pass -- the kernel gives no order among the lanes of a pass.  check() asserts it record by record; run() executes the program
with reads-then-writes semantics per pass, which is what any schedule that keeps the contract computes, so its rows and its violation
count can be compared with tests/wplan_ref.py independently of both kernels.  (Which producer a reader of a slot MEANS is not in the
record; check() asserts that the slot was written in an earlier pass and reports its last writer, run() then shows whether the value in
it is the right one.)"""
from typing import NamedTuple

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RINV = pow(1 << 256, R - 2, R)
WORDS, T = 19, 8
NOP, DOT, STEP, HINT = 0, 1, 2, 3


class Src(NamedTuple):
    kind: int        # 0: + v, 1: - v, 2: + coef v, 3: + coef (a constant; `index` is the coefficient's)
    in_lds: bool
    index: int       # an LDS slot of the group, a variable of the witness row, or (kind 3) a coefficient
    coef: int        # kind 2: the coefficient's index


class Rec(NamedTuple):
    op: int
    sources: tuple   # what the kernel fetches: the terms of a DOT, the operands a, b, c of a STEP that are not empty (None where one is), the HINT's source
    slot: object     # the LDS slot written, or None
    target: object   # STEP: the variable written (None: a check)
    inv: object      # STEP: coefficient index of 1 / c_t, or None
    hint: object     # HINT: (kind 0 bits / 1 inverse / 2 non-zero, first variable, count, first bit)


def src_of(w0, w1):
    return Src(w0 >> 30, bool((w0 >> 29) & 1), w0 & 0x0fffffff, w1)


def decode(records):
    """records: uint32 (passes + 1, 19, lanes) -> a list of passes, each a list of `lanes` Rec"""
    n_passes, words, lanes = records.shape
    assert words == WORDS
    out = []
    for p in range(n_passes):
        this = []
        for lane in range(lanes):
            w = [int(x) for x in records[p, :, lane]]
            head = w[0]
            op, n, slot = head & 15, (head >> 4) & 15, (head >> 16) - 1 if head >> 16 else None
            assert op in (NOP, DOT, STEP, HINT), (p, lane, op)
            if op == NOP:
                assert not any(w), (p, lane)
                this.append(Rec(NOP, (), None, None, None, None))
            elif op == DOT:
                assert 1 <= n <= T, (p, lane, n)
                this.append(Rec(DOT, tuple(src_of(w[3 + 2 * i], w[4 + 2 * i]) for i in range(n)), slot, None, None, None))
            elif op == STEP:
                e_a, e_b, e_c, check = (head >> 12) & 1, (head >> 13) & 1, (head >> 14) & 1, (head >> 9) & 1
                a, b, c = (src_of(w[3 + 2 * i], 0) for i in range(3))
                srcs = (None if e_a or e_b else a, None if e_a or e_b else b, None if e_c else c)       # a b is not evaluated when either is empty
                for s in srcs:
                    assert s is None or s.kind in (0, 3), (p, lane, s)                                 # fetch() applies no sign and no coefficient
                this.append(Rec(STEP, srcs, None if check else slot, None if check else w[1], w[2] if (head >> 8) & 1 and not check else None, None))
            else:
                hk = (head >> 10) & 3
                assert hk in (0, 1, 2), (p, lane)
                src = src_of(w[3], 0)
                assert src.kind == 0, (p, lane)
                this.append(Rec(HINT, (src,), slot if hk else None, None, None, (hk, w[1], w[2], w[4])))
        out.append(this)
    return out


def writes_of(rec):
    """(the slot written or None, the row variables written)"""
    if rec.op == DOT:
        return rec.slot, []
    if rec.op == STEP:
        return rec.slot, [] if rec.target is None else [rec.target]
    if rec.op == HINT:
        return rec.slot, list(range(rec.hint[1], rec.hint[1] + rec.hint[2]))
    return None, []


def check(passes, lanes, V, supplied, n_coefs):
    """the pass contract; raises AssertionError naming the pass and the lane"""
    assert passes and all(r.op == NOP for r in passes[-1]), "the program must end in an empty pass (the kernel reads one pass ahead)"
    n_slots = 32 * lanes
    slot_writer = {}                                                 # slot -> (pass, lane) of its last writer
    var_writer = {v: (-1, -1) for v in set(supplied) | {0}}          # variable -> where it was written; supplied: before the program
    for p, recs in enumerate(passes):
        assert len(recs) == lanes and sum(r.op != NOP for r in recs) <= lanes, p
        slots_read, vars_read, slots_written, vars_written = {}, {}, {}, {}
        for lane, r in enumerate(recs):
            for s in r.sources:
                if s is None:
                    continue
                if s.kind == 3:
                    assert s.index < n_coefs, (p, lane, "coefficient index")
                    continue
                if s.kind == 2:
                    assert r.op == DOT and s.coef < n_coefs, (p, lane, "coefficient index")
                if s.in_lds:
                    assert s.index < n_slots, (p, lane, "slot index", s.index)
                    assert s.index in slot_writer, (p, lane, "reads slot %d that nothing has written" % s.index)
                    slots_read.setdefault(s.index, lane)
                else:
                    assert s.index <= V, (p, lane, "variable index", s.index)
                    assert s.index in var_writer, (p, lane, "reads variable %d that is neither supplied nor written in an earlier pass" % s.index)
                    vars_read.setdefault(s.index, lane)
            if r.op == DOT:
                assert r.slot is not None, (p, lane, "a DOT without a slot loses its value")
            if r.inv is not None:
                assert r.inv < n_coefs, (p, lane)
            slot, variables = writes_of(r)
            if slot is not None:
                assert slot < n_slots, (p, lane, "slot index", slot)
                assert slot not in slots_written, (p, lane, "slot %d is written by lane %d as well" % (slot, slots_written.get(slot, -1)))
                slots_written[slot] = lane
            for v in variables:
                assert 0 < v <= V, (p, lane, "variable index", v)
                assert v not in var_writer and v not in vars_written, (p, lane, "variable %d is written twice" % v)
                vars_written[v] = lane
        for s, lane in slots_read.items():
            assert s not in slots_written, (p, "slot %d is read by lane %d and written by lane %d in one pass" % (s, lane, slots_written.get(s, -1)))
        for v, lane in vars_read.items():
            assert v not in vars_written, (p, "variable %d is read by lane %d and written by lane %d in one pass" % (v, lane, vars_written.get(v, -1)))
        for s, lane in slots_written.items():
            slot_writer[s] = (p, lane)
        for v, lane in vars_written.items():
            var_writer[v] = (p, lane)
    missing = [v for v in range(V + 1) if v not in var_writer]
    assert not missing, "variable %d is never written" % missing[0]


def check_bit_hints(passes, lanes, hints):
    """hints: (first, count) of every ZK_WHINT_BITS hint.  Its bits are split over at most `lanes` records, each a
    contiguous run first + bit0 .. of the bits, the runs covering 0 .. count - 1 once"""
    for first, count in hints:
        runs = [(p, r.hint[3], r.hint[2]) for p, recs in enumerate(passes) for r in recs
                if r.op == HINT and r.hint[0] == 0 and first <= r.hint[1] < first + count]
        assert 1 <= len(runs) <= min(lanes, count), (first, count, "bit hint split into %d records" % len(runs))
        at = 0
        for _, bit0, n in sorted(runs, key=lambda x: x[1]):
            assert bit0 == at and n >= 1, (first, count, bit0, at)
            at += n
        assert at == count, (first, count, at)
    for p, recs in enumerate(passes):
        for lane, r in enumerate(recs):
            if r.op == HINT and r.hint[0] == 0:
                assert r.hint[1] - r.hint[3] in {f for f, _ in hints}, (p, lane, "run of bits that belongs to no hint")


def run(passes, coefs, start):
    """the program over Python integers, reads first, then writes, pass by pass.  coefs: uint32 (n, 8) Montgomery limbs; start: the V + 1
    integers of a start row.  Returns (the row, violated checks)."""
    cf = [sum(int(x) << (32 * i) for i, x in enumerate(c)) * RINV % R for c in coefs]
    w = [x % R for x in start]
    slots = {}
    bad = 0

    def fetch(s):
        return cf[s.index] if s.kind == 3 else slots[s.index] if s.in_lds else w[s.index]

    for recs in passes:
        put_slots, put_vars = {}, {}
        for r in recs:
            if r.op == DOT:
                acc = 0
                for s in r.sources:
                    v = fetch(s)
                    if s.kind == 2:
                        v = cf[s.coef] * v
                    acc += -v if s.kind == 1 else v
                put_slots[r.slot] = acc % R
            elif r.op == STEP:
                a, b, c = r.sources
                v = fetch(a) * fetch(b) if a is not None else 0
                if c is not None:
                    v -= fetch(c)
                v %= R
                if r.target is None:
                    bad += v != 0
                    continue
                if r.inv is not None:
                    v = v * cf[r.inv] % R
                put_vars[r.target] = v
                if r.slot is not None:
                    put_slots[r.slot] = v
            elif r.op == HINT:
                hk, first, count, bit0 = r.hint
                x = fetch(r.sources[0])
                if hk == 0:
                    for i in range(count):
                        put_vars[first + i] = (x >> (bit0 + i)) & 1 if bit0 + i < 256 else 0
                else:
                    v = pow(x, R - 2, R) if hk == 1 else int(x != 0)
                    put_vars[first] = v
                    if r.slot is not None:
                        put_slots[r.slot] = v
        slots.update(put_slots)
        for v, x in put_vars.items():
            w[v] = x
    return w, bad
