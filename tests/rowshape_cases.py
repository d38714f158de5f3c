"""Satisfiable constraint systems with PRESCRIBED ROW SHAPES for the R1CS row evaluation (DevCsr::upload / DevCsr::enqueue in csrc/zkhip.cpp,
k_spmv_rows / k_spmv_long_chunks / k_spmv_long_finish in csrc/ntt.hpp).  Pure Python over big ints.

generate() takes the number of terms of every row of A, of B and of C, nIn, a coefficient mode and a seed.  Row j draws its columns from the
variables that exist when it is written -- 0 (ONE), the free variables 1 .. n_free, the variables the rows before it defined, and V, a free
variable that lies at the END of the witness so that the last column is read by rows everywhere -- with repetition.  The last term of C_j is a
fresh variable with a non-zero coefficient k_j, solved as x_new = (<A_j, w> <B_j, w> - rest) / k_j; an empty A_j or B_j makes the product 0 and
the fresh variable makes the row 0; an empty C_j is accepted only there.  The system depends on (shape, nIn, mode, seed, forced, late) alone:
witness() solves the same system again for other values of the free variables, as `witness_seed` of r1cs.random_r1cs does.

Why these lengths: a row of up to SPMV_LONG_ROW = 64 terms is summed by one thread, a longer one is cut into chunks of SPMV_CHUNK = 4 096
terms, one workgroup each, and a workgroup per long row adds its chunks' sums.  64 | 65, 4 096 | 4 097, 8 192 | 8 193 are the lengths at which
the path or the number of chunks changes; 12 289 = 3 chunks and one term."""
import functools
from collections import namedtuple
from ethsnarks_amd import r1cs as R
from ethsnarks_amd.fields import FR

LONG_ROW, CHUNK = 64, 4096                       # SPMV_LONG_ROW, SPMV_CHUNK of csrc/ntt.hpp
MODES = ("one", "general", "mix")
LENGTHS = (0, 1, 63, 64, 65, 66, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 12289)

System = namedtuple("System", "r1cs rows_a rows_b rows_c n_free late")


def chunks_of(n):
    return 0 if n <= LONG_ROW else (n + CHUNK - 1) // CHUNK


def _coefficient(rng, mode, nonzero=False):
    if mode == "one":
        return 1
    if mode == "general":
        return rng.fr() or 1
    pick = rng.next() % 4                        # "mix": ONE, 0, r - 1 and general side by side in one row
    if pick == 1 and not nonzero:
        return 0
    return (1, FR - 1, FR - 1, rng.fr() or 1)[pick]


def generate(counts_a, counts_b, counts_c, nIn, mode, seed, forced=False, late=None):
    """-> System.  forced: every row of three terms or more starts (0, 7), (V, .) and ends on the column of its third term -- column 0 with a
    coefficient other than one, the last column, a repeated column.  late = (matrix, row): the free variable n_free is kept out of every draw
    and stands once, with coefficient 1, at term CHUNK + 5 of that row: only the row's second chunk reads it."""
    assert mode in MODES and len(counts_a) == len(counts_b) == len(counts_c)
    nC = len(counts_a)
    rng = R.SplitMix64(seed)
    n_free = nIn + 2 + (1 if late else 0)
    V = n_free + sum(1 for n in counts_c if n) + 1
    rows = ([], [], [])
    nv = n_free + 1                              # columns 0 .. nv - 1 exist, and column V
    for j in range(nC):
        n_draw = nv - 1 if late else nv          # (the late variable, the last free one, is skipped)

        def draw(n, q):
            def column():
                i = rng.next() % (n_draw + 1)
                return V if i == n_draw else i + 1 if late and i >= n_free else i
            row = [(column(), _coefficient(rng, mode)) for _ in range(n)]
            if forced and n >= 3:
                row[0] = (0, 7)
                row[1] = (V, row[1][1])
                row[-1] = (row[2][0], row[-1][1])
            if late == (q, j):
                assert n > CHUNK + 5
                row[CHUNK + 5] = (n_free, 1)
            return row
        na, nb, nc = counts_a[j], counts_b[j], counts_c[j]
        assert nc or not (na and nb), ("row %d: an empty C needs an empty A or B" % j)
        rows[0].append(draw(na, 0))
        rows[1].append(draw(nb, 1))
        rc = draw(nc - 1, 2) if nc else []
        if nc:
            rc.append((nv, _coefficient(rng, mode, nonzero=True)))
            nv += 1
        rows[2].append(rc)
    assert nv == V
    r = R.R1CS(nC, nIn, V, R.CSR.from_rows(rows[0]), R.CSR.from_rows(rows[1]), R.CSR.from_rows(rows[2]))
    for q, counts in enumerate((counts_a, counts_b, counts_c)):
        assert [len(x) for x in rows[q]] == list(counts)
    return System(r, rows[0], rows[1], rows[2], n_free, late)


def dot(row, w):
    return sum(c * w[i] for i, c in row) % FR


def witness(s, witness_seed=None, edge=None):
    """the witness of system s whose free variables (1 .. n_free and V) are drawn from witness_seed, or are an edge: "zero" all 0, "rm1" all
    r - 1, "alternate" 0, r - 1, 0, ...  Solved row by row; asserted to satisfy the system."""
    V = s.r1cs.V
    rng = R.SplitMix64(witness_seed if witness_seed is not None else 1)
    free = list(range(1, s.n_free + 1)) + [V]
    value = {None: lambda i: rng.fr(), "zero": lambda i: 0, "rm1": lambda i: FR - 1, "alternate": lambda i: (0, FR - 1)[i & 1]}[edge]
    w = [None] * (V + 1)
    w[0] = 1
    for i, v in enumerate(free):
        w[v] = value(i)
    for ra, rb, rc in zip(s.rows_a, s.rows_b, s.rows_c):
        if not rc:
            continue
        col, k = rc[-1]
        assert w[col] is None and k % FR
        w[col] = (dot(ra, w) * dot(rb, w) - dot(rc[:-1], w)) * pow(k, -1, FR) % FR
    assert all(v is not None for v in w)
    return w


# ---------------------------------------------------------------- the directed cases
def _short(j, salt):
    return 1 + (j * 7 + salt) % 4


def _shape(nC, layout_a, layout_b, layout_c):
    out = []
    for q, layout in enumerate((layout_a, layout_b, layout_c)):
        out.append([layout.get(j, _short(j, q)) for j in range(nC)])
    for j in range(nC):                          # an empty C only where the product is 0
        assert out[2][j] or not (out[0][j] and out[1][j]), j
    return out


N_LEN = 300                                      # rows of the row-length cases: the long rows lie in both workgroups of k_spmv_rows


def _row_lengths():
    """every length of LENGTHS once in every matrix, no two matrices alike.  A: a long row at row 0, 64 | 65 next to each other, three long
    rows in a row (2, 3, 4), a pair across the workgroup boundary of k_spmv_rows (255, 256, 257), the last row.  B: 12 289 between two short
    rows, pairs (6, 7) and (N - 2, N - 1).  C: long rows at 0 and N - 1, a run of five from 200, an empty row where A's row is empty."""
    n = N_LEN
    a = {0: 4097, 1: 64, 2: 65, 3: 8193, 4: 4096, 10: 0, 11: 1, 12: 63, 13: 66, 100: 255, 101: 256, 102: 257, 255: 4095, 256: 8192, n - 1: 12289}
    b = {0: 66, 1: 12289, 2: 64, 5: 65, 6: 4096, 7: 4097, 20: 0, 21: 1, 22: 63, 150: 257, 151: 255, 152: 256, 254: 8192, n - 2: 4095, n - 1: 8193}
    c = {0: 8193, 1: 1, 2: 63, 3: 64, 4: 65, 10: 0, 30: 66, 31: 255, 60: 256, 61: 257, 200: 4095, 201: 4096, 202: 4097, 203: 12289, n - 1: 8192}
    for layout in (a, b, c):
        assert sorted(layout.values()) == sorted(LENGTHS)
    return _shape(n, a, b, c)


def _c_only():
    """long rows in C and nowhere else: one, two, three and four chunks, at row 0, next to each other and at the last row"""
    n = 40
    return _shape(n, {}, {}, {0: 4097, 17: 65, 18: 8193, 19: 4096, n - 1: 12289})


N_MANY = 70


def _many_long():
    """70 long rows of 1, 2, 3, 1, 2, 3, ... chunks in A -- more long rows than a wave has lanes, long_first with unequal strides -- the first
    40 next to each other from row 1, the rest on every third row; two long rows in B and one in C, so that three chunk plans differ"""
    n = 150
    lengths = (65, 4097, 8193)
    at = list(range(1, 41)) + list(range(50, 50 + 3 * 30, 3))
    assert len(at) == N_MANY and at[-1] < n
    a = {j: lengths[i % 3] for i, j in enumerate(at)}
    return _shape(n, a, {3: 4096, 149: 130}, {70: 8192})


PADDING = ((255, 0), (256, 0), (250, 5), (251, 5), (3, 300), (256, 255))      # (nC, nIn): short rows only


def _padding(nC, nIn):
    return _shape(nC, {}, {}, {})


#         name: (shape, nIn, mode, seed, forced)
CASES = {"lengths_%s" % mode: (_row_lengths, 2, mode, 11 + i, True) for i, mode in enumerate(MODES)}
CASES["c_only"] = (_c_only, 1, "general", 21, False)
CASES["many_long"] = (_many_long, 1, "general", 22, False)
for _nC, _nIn in PADDING:
    CASES["padding_%d_%d" % (_nC, _nIn)] = (functools.partial(_padding, _nC, _nIn), _nIn, "general", 30 + _nC + _nIn, False)
LENGTH_CASES = tuple("lengths_%s" % mode for mode in MODES)
PADDING_CASES = tuple("padding_%d_%d" % p for p in PADDING)
ROW_CASES = LENGTH_CASES + ("c_only", "many_long") + PADDING_CASES
PROOF_CASES = ("lengths_general", "many_long") + PADDING_CASES

LATE_ROW = (0, 3)                                # A's row 3 of the row-length layout: 8 193 terms, three chunks
LATE_SEED = 41


@functools.lru_cache(maxsize=None)
def system(name):
    if name == "late":                           # the row-length system with one variable that only the second chunk of A's row 3 reads
        s = generate(*_row_lengths(), nIn=2, mode="general", seed=LATE_SEED, forced=True, late=LATE_ROW)
    else:
        shape, nIn, mode, seed, forced = CASES[name]
        s = generate(*shape(), nIn=nIn, mode=mode, seed=seed, forced=forced)
    check_reaches(name, s)
    return s


@functools.lru_cache(maxsize=None)
def witnesses(name):
    """{label: witness ints} of a case, computed once: two random ones and the edges.  Every one satisfies the system."""
    s = system(name)
    out = {"a": witness(s, 101), "b": witness(s, 202), "zero": witness(s, edge="zero"), "rm1": witness(s, edge="rm1"), "alternate": witness(s, edge="alternate")}
    for label, w in out.items():
        assert s.r1cs.is_satisfied(w), (name, label)
    assert len({tuple(w) for w in out.values()}) == len(out)
    return out


def check_reaches(name, s):
    """every case reaches the edge it is there for (asserted on the system that is returned, not on the request)"""
    r = s.r1cs
    lens = [[int(x) for x in (m.row_ptr[1:].astype("int64") - m.row_ptr[:-1].astype("int64"))] for m in (r.A, r.B, r.C)]
    longs = [[j for j, n in enumerate(l) if n > LONG_ROW] for l in lens]
    if name.startswith("lengths") or name == "late":
        assert all(set(LENGTHS) <= set(l) for l in lens)
        assert lens[0] != lens[1] != lens[2] != lens[0]
        assert 0 in longs[0] and r.nC - 1 in longs[0] and 0 in longs[2] and r.nC - 1 in longs[2]                    # row 0, the last row
        assert all(any(j + 1 in l for j in l) for l in longs)                                                     # adjacent pairs
        assert lens[0][1] == 64 and lens[0][2] == 65                                                              # short next to long
        assert all(len({chunks_of(lens[q][j]) for j in longs[q]}) >= 4 for q in range(3))                         # 1, 2, 3 and 4 chunks in one plan
        assert all(any(j >= 256 for j in l) and any(j < 256 for j in l) for l in longs)                           # both workgroups of k_spmv_rows
        for rows in (s.rows_a, s.rows_b, s.rows_c):
            big = [row for row in rows if len(row) > LONG_ROW]
            assert all(row[0] == (0, 7) and row[1][0] == r.V for row in big)                                      # column 0 x 7, column V
            assert all(len({c for c, _ in row}) < len(row) for row in big)                                        # repeated columns
        mode = "general" if name == "late" else name.split("_")[1]
        coefs = {k for rows in (s.rows_a, s.rows_b, s.rows_c) for row in rows if len(row) > CHUNK for _, k in row[2:]}
        if mode == "one":
            assert coefs == {1}
        elif mode == "mix":
            assert {0, 1, FR - 1} < coefs
        else:
            assert len(coefs) > 1000
    if name == "late":
        q, j = s.late
        hits = [(qq, jj, t) for qq, rows in enumerate((s.rows_a, s.rows_b, s.rows_c)) for jj, row in enumerate(rows) for t, (c, _) in enumerate(row) if c == s.n_free]
        assert hits == [(q, j, CHUNK + 5)] and chunks_of(lens[q][j]) == 3
    if name == "c_only":
        assert not longs[0] and not longs[1] and len(longs[2]) == 5
    if name == "many_long":
        assert len(longs[0]) == N_MANY and [chunks_of(lens[0][j]) for j in longs[0]] == [1 + i % 3 for i in range(N_MANY)]
    if name.startswith("padding"):
        assert not any(longs) and (r.nC, r.nIn) in PADDING
        total = r.nC + r.nIn + 1                                     # what each pair is there for
        why = {(255, 0): total == 256, (256, 0): r.nC % 256 == 0 and total == 257, (250, 5): total == 256 and r.nC + r.nIn == 255,
               (251, 5): total == 257, (3, 300): r.nIn + 1 > 256, (256, 255): r.nC % 256 == 0 and total == 512}
        assert why[(r.nC, r.nIn)]
    m = r.domain_size
    assert m <= 1024 and r.V <= 700
