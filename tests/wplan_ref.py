"""Reference for the witness plans (zk_wplan_create_hinted, zk_wplan_create_wide): forward substitution over plain Python integers mod r,
written from the definition in include/zkhip.h.  It shares no code with ethsnarks_amd/prover.py, the gadgets or the C sources.

A system is rows_a, rows_b, rows_c (one list of (column, int coefficient) pairs per constraint; column 0 is the constant ONE), the number of
variables V, the supplied columns, and hints (kind, src, first, count) with the kinds of include/zkhip.h.  The constraints are walked in
order.  A column that is still unknown when a constraint reads it may be defined by its hint, if the hint's source is known by then.  What is
then still unknown in C is the constraint's target: w[t] = (<A, w> <B, w> - C_rest) / c_t.  A constraint with no unknown is a check."""

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

BITS, INV, NONZERO = 1, 2, 3


class NotSolvable(Exception):
    pass


def hint_values(kind, src_value, count):
    v = src_value % R
    if kind == BITS:
        return [(v >> i) & 1 if i < 256 else 0 for i in range(count)]
    if kind == INV:
        return [pow(v, R - 2, R)]                                     # 0 for 0
    if kind == NONZERO:
        return [1 if v else 0]
    raise NotSolvable("unknown hint kind %r" % (kind,))


def solve(rows_a, rows_b, rows_c, V, supplied, hints, start):
    """start: V + 1 integers, the supplied columns filled in (the others are ignored).  Returns (the full row, violated checks)."""
    w = [None] * (V + 1)
    for v in set(supplied) | {0}:
        w[v] = start[v] % R
    hint_of = {}
    for h, (kind, src, first, count) in enumerate(hints):
        for i in range(count):
            hint_of[first + i] = h
    fired = set()

    def know(col):
        if w[col] is None and col in hint_of and hint_of[col] not in fired:
            kind, src, first, count = hints[hint_of[col]]
            if w[src] is not None:
                for i, bit in enumerate(hint_values(kind, w[src], count)):
                    w[first + i] = bit
                fired.add(hint_of[col])
        return w[col] is not None

    def dot(row):
        return sum(c * w[col] for col, c in row) % R

    bad = 0
    for j, (ra, rb, rc) in enumerate(zip(rows_a, rows_b, rows_c)):
        for row in (ra, rb):
            for col, _ in row:
                if not know(col):
                    raise NotSolvable("constraint %d reads column %d before it is defined" % (j, col))
        target, tcoef, rest = None, 0, []
        for col, c in rc:
            if know(col):
                rest.append((col, c))
            elif target is None:
                target, tcoef = col, c % R
            else:
                raise NotSolvable("constraint %d has two unknowns (%d and %d)" % (j, target, col))
        ab = dot(ra) * dot(rb) % R
        if target is None:
            bad += (ab - dot(rest)) % R != 0
        else:
            if tcoef == 0:
                raise NotSolvable("constraint %d: zero coefficient on its target" % j)
            w[target] = (ab - dot(rest)) * pow(tcoef, R - 2, R) % R
    missing = [v for v in range(V + 1) if w[v] is None]
    if missing:
        raise NotSolvable("column %d is never defined" % missing[0])
    return w, bad
