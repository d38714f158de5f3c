"""Constraint systems for the witness-plan checks (wplan_fuzz_checks.py): seeded builders of directed systems, one feature each so that a
failure names it, and a generator that strings the same shapes together.  Nothing here computes a witness: tests/wplan_ref.py does.

A builder returns a Case: (rows_a, rows_b, rows_c, V, supplied, hints) and, as a seventh field, `echo`: {supplied column: derived column}.
An echo column is read by check constraints only and must be given the value the reference finds for its derived column; start_rows() does
that, and then changes it in some rows, so that the expected number of violated checks is non-zero and is the reference's."""
import functools
import random
from typing import NamedTuple
import wplan_ref as ref

R = ref.R
LANES = (4, 8, 16, 32, 64)
WW_T, WW_REUSE = 8, 32                                               # csrc/wplan_wide.hpp


class Case(NamedTuple):
    rows_a: list
    rows_b: list
    rows_c: list
    V: int
    supplied: list
    hints: list
    echo: dict


class Sys:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.a, self.b, self.c = [], [], []
        self.n = 1
        self.supplied, self.hints, self.echo = [0], [], {}
        self.last = None

    def var(self):
        self.n += 1
        return self.n - 1

    def sup(self, n):
        out = [self.var() for _ in range(n)]
        self.supplied += out
        return out

    def add(self, a, b, c, target=None):
        self.a.append(list(a)); self.b.append(list(b)); self.c.append(list(c))
        if target is not None:
            self.last = target
        return len(self.a) - 1

    def define(self, a, b, rest=(), coef=1, at=None):
        """a new variable t with <a><b> = rest + coef t; the target's term sits at position `at` of the C row (default: last)"""
        t = self.var()
        c = list(rest)
        c.insert(len(c) if at is None else at, (t, coef))
        self.add(a, b, c, t)
        return t

    def mul(self, x, y):
        return self.define([(x, 1)], [(y, 1)])

    def general(self):
        return self.rng.randrange(3, R - 1)

    def coef(self):
        return self.rng.choice([1, -1, 0, 2, self.general(), self.general()])

    def row(self, cols, n, one_at=None):
        """n terms over `cols` (cycled, so a row longer than the pool repeats columns), coefficients from {1, -1, 0, 2, random}"""
        out = [(cols[(i * 5 + i // len(cols)) % len(cols)], self.coef()) for i in range(n)]
        if one_at is not None and n:
            out[one_at] = (0, self.general())
        return out

    def echo_check(self, t):
        e = self.sup(1)[0]
        self.echo[e] = t
        self.add([(e, 1)], [(0, 1)], [(t, 1)])
        return e

    def violated_check(self, t):
        self.add([(t, 1)], [(0, 1)], [(t, 1), (0, 1)])               # t = t + 1: never holds

    def done(self):
        if self.last is not None:
            self.echo_check(self.last)
        return Case(self.a, self.b, self.c, self.n - 1, list(self.supplied), list(self.hints), dict(self.echo))


# ---------------------------------------------------------------- directed: row lengths
ROW_LENGTHS = (0, 1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 512, 513)


def row_length(n):
    s = Sys(1000 + n)
    pool = s.sup(min(max(n, 3), 24))
    ra, rb, rc = (s.row(pool, n, one_at=n // 2 if n >= 3 else None) for _ in range(3))
    t1 = s.define(ra, [(pool[0], 1)])
    t2 = s.define([(pool[1], 1)], rb, coef=-1)
    t3 = s.define([(t1, 1)], [(t2, 1)], rest=rc, coef=s.general())
    if 3 * -(-n // WW_T) <= 100:                                     # (the chunk temporaries of one constraint wait together: 4 lanes have 128 slots)
        s.define(ra, rb, rest=rc)                                    # all three long, the rows met again
        s.define([(t3, 1)], rc, rest=ra, coef=-1, at=n // 2)
    else:
        s.define([(t3, 1)], [(t1, 1)], rest=ra, coef=-1, at=n // 2)
    return s.done()


def row_first_minus_one():
    s = Sys(1100)
    p = s.sup(6)
    row = [(p[0], 0), (p[1], -1), (p[2], 5), (p[3], 1), (p[4], -1)]
    t = s.define(row, [(p[5], 1)])
    u = s.define([(t, -1)], [(p[0], -1)], rest=[(p[2], 0), (p[1], -1), (p[0], 1)])      # lone -v as A and as B
    s.define([(p[0], 0), (0, 0), (u, -1), (t, -1)], [(0, 0), (u, -1)], rest=[(0, 0), (t, -1)])
    return s.done()


def row_all_zeros():
    s = Sys(1101)
    p = s.sup(4)
    t = s.define([(p[0], 0), (p[1], 0), (0, 0)], [(p[2], 1)], rest=[(p[3], 1)])         # A sums to nothing: t = -p3
    u = s.define([(p[2], 1)], [(p[0], 0)], rest=[(p[1], 0), (0, 0)], coef=3)            # B and the rest of C are zeros: u = 0
    s.define([(t, 1)], [(p[0], 2)], rest=[(u, 0)] * 9)
    s.add([(u, 1)], [(p[1], 1)], [(p[2], 0)])                                         # a check that holds: 0 = 0
    return s.done()


def row_duplicate_column():
    s = Sys(1102)
    p = s.sup(3)
    row = [(p[0], 3), (p[0], 1), (p[0], -1), (p[1], 2), (p[0], 3), (0, 4), (0, -4), (0, 9), (p[1], -2)]
    t = s.define(row, row)
    s.define([(t, 1), (t, 1), (t, -1)], [(p[2], 1), (p[2], 1)], rest=[(t, 1), (t, 7), (p[0], 1), (t, -1)], coef=-1, at=2)
    return s.done()


def row_one_in_the_middle():
    s = Sys(1103)
    p = s.sup(20)
    row = s.row(p, 41)
    row[20] = (0, s.general()); row[3] = (0, 1); row[33] = (0, -1)
    t = s.define(row, [(0, 5)])                                                        # B a lone constant
    s.define([(0, 1)], row, rest=[(t, 1), (0, 6), (p[0], 1)], coef=2, at=1)
    return s.done()


# ---------------------------------------------------------------- directed: operand shapes
def shape(name):
    s = Sys(1200 + sorted(SHAPES).index(name))
    p = s.sup(6)
    g, lrow = s.general(), None
    rest3 = [(p[3], 2), (0, 7), (p[4], -1)]
    if name == "a_empty":
        s.define([], [(p[0], 1), (p[1], 3)], rest=[(p[2], 1), (0, 3)], coef=g)
    elif name == "b_empty_a_long":
        lrow = s.row(p, 40, one_at=11)
        s.define(lrow, [], rest=[(p[2], 5)], coef=-1)
    elif name == "both_empty":
        t = s.define([], [], rest=rest3)
        s.define([], [], coef=g)                                                       # g t = 0
        s.add([], [], [(t, 1)] + rest3)                                                # a check that holds: 0 = t + rest
    elif name == "c_rest_empty":
        s.define([(p[0], 1), (p[1], g)], [(p[2], -1)])
    elif name == "c_rest_lone_var":
        s.define([(p[0], 1)], [(p[1], 1)], rest=[(p[2], 1)])
    elif name == "c_rest_lone_const":
        s.define([(p[0], 1)], [(p[1], 1)], rest=[(0, g)])
    elif name == "c_rest_lone_minus_var":
        s.define([(p[0], 1)], [(p[1], 1)], rest=[(p[2], -1)], coef=g)
    elif name in ("target_first", "target_middle", "target_last"):
        at = {"target_first": 0, "target_middle": 2, "target_last": None}[name]
        for coef in (1, -1, g):
            s.define([(p[0], 1), (p[5], 1)], [(p[1], 1)], rest=rest3 + [(p[2], g)], coef=coef, at=at)
    elif name in ("target_coef_one", "target_coef_minus_one", "target_coef_general"):
        coef = {"target_coef_one": 1, "target_coef_minus_one": -1, "target_coef_general": g}[name]
        t = s.define([(p[0], 1)], [(p[1], 1)], coef=coef)
        t = s.define([(t, 1)], [(t, 1)], rest=[(p[2], 1)], coef=coef)
        s.define([(t, 2), (p[0], 1)], [(t, 1)], rest=rest3, coef=coef, at=1)
    else:
        raise KeyError(name)
    return s.done()


SHAPES = {"a_empty", "b_empty_a_long", "both_empty", "c_rest_empty", "c_rest_lone_var", "c_rest_lone_const", "c_rest_lone_minus_var",
          "target_first", "target_middle", "target_last", "target_coef_one", "target_coef_minus_one", "target_coef_general"}


# ---------------------------------------------------------------- directed: row reuse
def dots_of(n_terms):
    """DOT operations that evaluate one combination of n surviving terms: chunks of WW_T, then a DOT over their temporaries, and so on"""
    dots = 0
    while n_terms > WW_T:
        n_terms = -(-n_terms // WW_T)
        dots += n_terms
    return dots + 1


def reuse_same_row_abc():
    s = Sys(1300)
    p = s.sup(12)
    row = [(p[i % 12], 3 + i) for i in range(20)]
    s.define(row, row, rest=row)
    return s.done(), dots_of(20)


def reuse_at_distance(d, change=False):
    """the 20-term row in constraint 0 and in constraint d; a chain of lone-variable products between them (no DOTs of their own)"""
    s = Sys(1310 + d + 100 * change)
    p = s.sup(12)
    row = [(p[i % 12], 3 + i) for i in range(20)]
    x = s.define(row, [(p[0], 1)])
    for _ in range(d - 1):
        x = s.mul(x, p[1])
    again = list(row)
    if change:
        again[13] = (again[13][0], again[13][1] + 1)
    s.define(again, [(x, 1)])
    return s.done(), dots_of(20) * (2 if change or d > WW_REUSE else 1)


# ---------------------------------------------------------------- directed: pass splitting
def pass_split(lanes):
    """four levels of lanes - 1, lanes, lanes + 1 and 3 lanes independent single-variable products"""
    s = Sys(1400 + lanes)
    prev = s.sup(5)
    for n in (lanes - 1, lanes, lanes + 1, 3 * lanes):
        prev = [s.mul(prev[i % len(prev)], prev[(i + 1) % len(prev)]) for i in range(n)]
    s.define([(v, 1) for v in prev], [(0, 1)])                       # every product of the last level is read
    return s.done()


# ---------------------------------------------------------------- directed: slot pressure
def slot_pressure(reverse):
    s = Sys(1500 + reverse)
    p = s.sup(8)
    n = 160
    f = [s.mul(p[i % 8], p[(3 * i + 1) % 8]) for i in range(n)]
    x = p[0]
    for k in range(24):
        x = s.define([(x, 1), (p[k % 8], 3)], [(x, 1), (p[(k + 1) % 8], -1)], coef=7 if k % 2 else 1)
    for i in range(n):
        fi = f[n - 1 - i] if reverse else f[i]
        x = s.define([(fi, 1)], [(x, 1)], rest=[(f[7 * i % n], 5)], coef=-1)
    s.violated_check(x)
    return s.done()


def eviction_in_the_pass_that_fills_the_pool(lanes):
    """32 lanes + 2 products at level 1.  The first 32 lanes fill the pool.  The last pass makes X, read late (only the product before it
    is read later, and loses its slot to X), and Y, read first: Y needs a slot, and the cached variable with the farthest next read is X,
    which the same pass writes -- X must keep its slot until the barrier, so Y has to take another one."""
    s = Sys(1550 + lanes)
    p = s.sup(7)
    n = 32 * lanes
    f = [s.mul(p[i % 7], p[(2 * i + 1) % 7]) for i in range(n + 2)]
    x = p[0]
    for v in [f[n + 1]] + f[:n - 1] + [f[n], f[n - 1]]:              # Y, the pool but its last product, X, that last product
        x = s.define([(v, 1)], [(x, 1)], rest=[(p[1], 1)])
    return s.done()


def refused_level():
    """160 independent constraints whose A and B are two-term rows: 320 temporaries at level 1"""
    s = Sys(1600)
    p = s.sup(9)
    for i in range(160):
        s.define([(p[i % 9], 2 + i), (p[(i + 1) % 9], 3)], [(p[(i + 2) % 9], 5), (p[(i + 4) % 9], 7 + i)])
    return s.done()


# ---------------------------------------------------------------- directed: hints
BIT_COUNTS = tuple(sorted({1, 3, 253, 254, 257} | {l + d for l in LANES for d in (-1, 0, 1)}))


def bits(count):
    s = Sys(1700 + count)
    x = s.sup(1)[0]
    first = s.n
    b = [s.var() for _ in range(count)]
    s.hints.append((ref.BITS, x, first, count))
    s.define([(v, pow(2, i, R)) for i, v in enumerate(b)], [(0, 1)])                    # the recomposition reads every bit
    s.add([(b[0], 1)], [(0, 1), (b[0], -1)], [])                                      # b (1 - b) = 0
    s.add([(b[-1], 1)], [(0, 1), (b[-1], -1)], [])
    return s.done()


def hint_source_is_derived():
    s = Sys(1800)
    p = s.sup(2)
    x = s.define([(p[0], 1), (0, 3)], [(p[1], 1)], coef=s.general())
    first = s.n
    b = [s.var() for _ in range(40)]
    s.hints.append((ref.BITS, x, first, 40))
    m, y = s.var(), s.var()
    s.hints.append((ref.INV, x, m, 1))
    s.hints.append((ref.NONZERO, x, y, 1))
    s.define([(v, 1 + i) for i, v in enumerate(b)], [(m, 1)], rest=[(y, 1)])
    return s.done()


def inv_feeds_nonzero():
    s = Sys(1801)
    p = s.sup(1)
    m, y, m2 = s.var(), s.var(), s.var()
    s.hints.append((ref.NONZERO, m, y, 1))                           # listed before the hint that defines its source
    s.hints.append((ref.INV, p[0], m, 1))
    s.hints.append((ref.INV, m, m2, 1))
    t = s.define([(m, 1)], [(p[0], 1)], rest=[(y, -1)])              # x / x - [1 / x != 0]: 0 whatever x is
    s.define([(m2, 1)], [(y, 1)], rest=[(t, 1)])
    return s.done()


def hinted_first_read_in(where):
    s = Sys(1810 + "ABC".index(where))
    p = s.sup(2)
    first = s.n
    b = [s.var() for _ in range(5)]
    s.hints.append((ref.BITS, p[0], first, 5))
    m = s.var()
    s.hints.append((ref.INV, p[1], m, 1))
    hinted = [(b[0], 1), (m, 3), (b[4], -1)]
    known = [(p[0], 1), (p[1], 2)]
    if where == "A":
        s.define(hinted, known)
    elif where == "B":
        s.define(known, hinted)
    else:
        s.define(known, known, rest=hinted, at=1)
    s.define([(b[2], 1)], [(m, 1)])
    return s.done()


def inv_nonzero_of_special_values():
    """INV and NONZERO of 0, 1 and r - 1, derived so that every start row meets them"""
    s = Sys(1820)
    p = s.sup(1)
    zero = s.define([(p[0], 1)], [])
    one = s.define([(0, 1)], [(0, 1)])
    minus_one = s.define([(0, 1)], [(0, 1)], coef=-1)
    outs = []
    for x in (zero, one, minus_one, p[0]):
        m, y = s.var(), s.var()
        s.hints.append((ref.INV, x, m, 1)); s.hints.append((ref.NONZERO, x, y, 1))
        outs += [(m, 2), (y, 3)]
        s.add([(x, 1)], [(m, 1)], [(y, 1)])                          # x m = y: holds for every x
    s.define(outs, [(0, 1)])
    return s.done()


# ---------------------------------------------------------------- the generator
def random_system(seed):
    """a few hundred constraints: chains, wide levels, long rows, repeated rows, hints and checks strung together.  Every segment reads the
    head of the chain, so the segments follow one another level by level and no level holds more than about 60 temporaries: at 4 lanes
    (128 slots) nothing is refused."""
    s = Sys(5000 + seed)
    rng = s.rng
    pool = s.sup(rng.randrange(3, 10))
    head = pool[0]
    recent_rows = []

    def short_row(extra, n):
        cols = [rng.choice(pool) for _ in range(n)]
        out = [(c, s.coef()) for c in cols]
        out.insert(rng.randrange(len(out) + 1), (extra, rng.choice([1, -1, s.general()])))
        if rng.random() < 0.2:
            out.insert(rng.randrange(len(out) + 1), (0, s.coef()))
        return out

    def tcoef():
        return rng.choice([1, 1, -1, 7, s.general()])

    while len(s.a) < 260:
        kind = rng.choice(["chain", "chain", "wide", "wide2", "long", "again", "bits", "inv", "check", "bad", "empty"])
        if kind == "chain":
            for _ in range(rng.randrange(3, 25)):
                rest = [(rng.choice(pool), s.coef()) for _ in range(rng.randrange(0, 4))]
                head = s.define(short_row(head, rng.randrange(0, 3)), short_row(head, rng.randrange(0, 3)), rest=rest, coef=tcoef(),
                                at=rng.randrange(len(rest) + 1))
                pool.append(head)
        elif kind == "wide":
            outs = [s.define([(head, rng.choice([1, 1, -1]))], [(rng.choice(pool), 1)],
                             rest=[(rng.choice(pool), 1)] if rng.random() < 0.3 else [], coef=tcoef()) for _ in range(rng.randrange(3, 70))]
            head = s.define([(v, s.coef() or 1) for v in outs], [(0, 1)])
            pool += outs[:6] + [head]
        elif kind == "wide2":
            outs = [s.define(short_row(head, 1), short_row(head, 2), coef=tcoef()) for _ in range(rng.randrange(2, 20))]
            head = s.define([(outs[-1], 1)], [(outs[0], 1)], rest=[(v, 2) for v in outs])
            pool += outs[:4] + [head]
        elif kind == "long":
            n = rng.choice([9, 17, 40, 63, 64, 65, 70, 130])
            row = s.row(pool[-40:], n, one_at=rng.randrange(n))
            recent_rows.append(row)
            where = rng.randrange(3)
            if where == 0:
                head = s.define(row, [(head, 1)], coef=tcoef())
            elif where == 1:
                head = s.define([(head, 1)], row, coef=tcoef())
            else:
                head = s.define([(head, 1)], [(head, 1)], rest=row, coef=tcoef(), at=rng.randrange(n + 1))
            pool.append(head)
        elif kind == "again" and recent_rows:
            row = list(rng.choice(recent_rows[-3:]))
            if rng.random() < 0.3:
                i = rng.randrange(len(row))
                row[i] = (row[i][0], row[i][1] + 1)
            head = s.define(row, row if rng.random() < 0.5 else [(head, 1)], rest=[(head, -1)], coef=tcoef())
            pool.append(head)
        elif kind == "bits":
            count = rng.choice([1, 2, 5, 9, 31, 33, 70])
            first = s.n
            b = [s.var() for _ in range(count)]
            s.hints.append((ref.BITS, head, first, count))
            head = s.define([(v, pow(2, i, R)) for i, v in enumerate(b)], [(head, 1)], coef=tcoef())
            s.add([(b[count // 2], 1)], [(0, 1), (b[count // 2], -1)], [])
            pool += b[:3] + [head]
        elif kind == "inv":
            m, y = s.var(), s.var()
            s.hints.append((ref.INV, head, m, 1)); s.hints.append((ref.NONZERO, head, y, 1))
            s.add([(head, 1)], [(m, 1)], [(y, 1)])
            head = s.define([(m, 1), (head, 1)], [(y, 1), (0, 2)], coef=tcoef())
            pool += [m, y, head]
        elif kind == "check":
            j = rng.randrange(len(s.a)) if s.a else None
            if j is not None:
                s.add(s.a[j], s.b[j], s.c[j])                        # a constraint met again introduces nothing: a check that holds
            if rng.random() < 0.5:
                s.echo_check(head)
        elif kind == "bad":
            s.violated_check(rng.choice(pool))
        elif kind == "empty":
            head = s.define([] if rng.random() < 0.5 else [(head, 0)], [(head, 1)], rest=[(head, -1), (0, s.general())], coef=tcoef())
            pool.append(head)
    s.last = head
    return s.done()


# ---------------------------------------------------------------- the registry, the start rows and the expected rows
DIRECTED = {}
EXPECTED_DOTS = {}
for _n in ROW_LENGTHS:
    DIRECTED["row_length_%d" % _n] = functools.partial(row_length, _n)
DIRECTED.update(row_first_minus_one=row_first_minus_one, row_all_zeros=row_all_zeros, row_duplicate_column=row_duplicate_column,
                row_one_in_the_middle=row_one_in_the_middle)
for _n in sorted(SHAPES):
    DIRECTED["shape_" + _n] = functools.partial(shape, _n)
for _l in LANES:
    DIRECTED["pass_split_%d" % _l] = functools.partial(pass_split, _l)
DIRECTED.update(slot_pressure_forward=functools.partial(slot_pressure, False), slot_pressure_reverse=functools.partial(slot_pressure, True))
for _l in (4, 8):
    DIRECTED["eviction_in_the_pass_that_fills_the_pool_%d" % _l] = functools.partial(eviction_in_the_pass_that_fills_the_pool, _l)
for _n in BIT_COUNTS:
    DIRECTED["bits_%d" % _n] = functools.partial(bits, _n)
DIRECTED.update(hint_source_is_derived=hint_source_is_derived, inv_feeds_nonzero=inv_feeds_nonzero,
                inv_nonzero_of_special_values=inv_nonzero_of_special_values)
for _w in "ABC":
    DIRECTED["hinted_first_read_in_" + _w] = functools.partial(hinted_first_read_in, _w)
REUSE = {"reuse_same_row_abc": reuse_same_row_abc, "reuse_at_distance_1": functools.partial(reuse_at_distance, 1),
         "reuse_at_distance_32": functools.partial(reuse_at_distance, 32), "reuse_at_distance_33": functools.partial(reuse_at_distance, 33),
         "reuse_changed_coefficient": functools.partial(reuse_at_distance, 1, True)}
for _name, _f in REUSE.items():
    DIRECTED[_name] = (lambda f: lambda: f()[0])(_f)


REFUSED_AT_FEW_LANES = {"refused_level": refused_level}             # not in DIRECTED: what runs at every lanes must be accepted at every lanes


@functools.lru_cache(maxsize=None)
def case(name):
    """a directed case by its name, or "seed_N": built once, never written to"""
    return random_system(int(name[5:])) if name.startswith("seed_") else {**DIRECTED, **REFUSED_AT_FEW_LANES}[name]()


def expected_dots(name):
    return REUSE[name]()[1]


MAX_ROWS = 67


@functools.lru_cache(maxsize=None)
def rows(name, n_rows):
    """for rows 0 .. n_rows - 1 of the case: (start values, the reference's full row, the reference's violation count).  The free supplied
    columns hold distinct draws from {0, 1, r - 1, random}; the echo columns hold what the reference finds for their derived columns, and
    in every third row (0, 3, ...) one of them is changed AFTER that, the row then being solved again: its count is not zero."""
    c = case(name)
    system = c[:6]
    rng = random.Random("rows of " + name)
    free = [v for v in c.supplied if v and v not in c.echo]
    out, seen = [], set()
    for p in range(n_rows):
        while True:
            vals = tuple(rng.choice([0, 1, R - 1, rng.randrange(R), rng.randrange(R)]) for _ in free)
            if vals not in seen or len(seen) >= 5 ** len(free) // 2:
                break
        seen.add(vals)
        start = [0] * (c.V + 1)
        start[0] = 1
        for v, x in zip(free, vals):
            start[v] = x
        full, bad = ref.solve(*system, start)
        for e, t in c.echo.items():
            start[e] = full[t]
        if p % 3 == 0 and c.echo:
            e = sorted(c.echo)[p // 3 % len(c.echo)]
            start[e] = (start[e] + 1 + p) % R
        full, bad = ref.solve(*system, start)
        out.append((start, full, bad))
    return out
