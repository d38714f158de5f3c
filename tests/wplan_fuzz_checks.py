"""Checks of both witness plans -- the tape (k_witness_tape) and the wide plan (k_witness_wide) at every `lanes` -- against the big-int solver
of wplan_ref.py on the systems of wplan_cases.py.  They run unchanged on the CPU stand-in (test_wplan_fuzz_emul.py) and on the device
(test_wplan_fuzz_gpu.py); `zk` is the ethsnarks_amd.prover module with a library loaded.  Everything is integer arithmetic: every element of
every row is compared byte for byte with fr_to_mont(reference), the sentinel row with what was uploaded, the violation count with the
reference's.  There is no tolerance anywhere."""
import contextlib
import functools
import os
import numpy as np
import pytest
from ethsnarks_amd import fields as F, r1cs as R
import wplan_cases as cases
import wplan_program as prog
import wplan_ref as ref

PLANS = (None,) + cases.LANES                                        # None: the tape plan


def r1cs_of(c):
    return R.R1CS(len(c.rows_a), 1, c.V, R.CSR.from_rows(c.rows_a), R.CSR.from_rows(c.rows_b), R.CSR.from_rows(c.rows_c))


def make_plan(zk, c, lanes, r=None):
    kw = dict(bit_hints=[(s, f, n) for k, s, f, n in c.hints if k == ref.BITS], inv_hints=[(s, f) for k, s, f, n in c.hints if k == ref.INV],
              nonzero_hints=[(s, f) for k, s, f, n in c.hints if k == ref.NONZERO])
    if lanes is not None:
        kw["lanes"] = lanes
    return zk.WitnessPlan(r or r1cs_of(c), c.supplied, **kw)


@functools.lru_cache(maxsize=None)
def arrays(name, n_rows):
    """(start rows, expected rows) in Montgomery form, (n_rows, V + 1, 4) each, and the expected violation count of every row: computed
    once, never written to"""
    rows = cases.rows(name, n_rows)
    V1 = len(rows[0][0])
    start = F.fr_to_mont([x for s, _, _ in rows for x in s]).reshape(n_rows, V1, 4)
    expect = F.fr_to_mont([x for _, e, _ in rows for x in e]).reshape(n_rows, V1, 4)
    start.setflags(write=False); expect.setflags(write=False)
    bads = tuple(b for _, _, b in rows)
    assert any(bads), name                                            # a changed echo column is a violated check in the reference
    return start, expect, bads


@contextlib.contextmanager
def lane_order(order):
    """the order in which the CPU stand-in runs the lanes of a block between two barriers (tests/emul/hip_emul.h); nothing on the device"""
    old = os.environ.get("ZK_EMUL_LANE_ORDER")
    os.environ["ZK_EMUL_LANE_ORDER"] = order
    try:
        yield
    finally:
        if old is None:
            del os.environ["ZK_EMUL_LANE_ORDER"]
        else:
            os.environ["ZK_EMUL_LANE_ORDER"] = old


def check_solves(zk, name, plans, ks_for, n_rows, orders=("ascending",)):
    """every plan of `plans` (None: the tape, else lanes) completes k rows for every k of ks_for(lanes): the rows, the sentinel row and the
    count are the reference's.  A refusal fails the test."""
    c = cases.case(name)
    start_all, expect_all, bads = arrays(name, n_rows)
    r = r1cs_of(c)
    for lanes in plans:
        plan = make_plan(zk, c, lanes, r)
        for k in ks_for(lanes):
            start = np.empty((k + 1, c.V + 1, 4), dtype=np.uint64)
            start[:k] = start_all[:k]
            start[k] = np.arange(4 * (c.V + 1), dtype=np.uint64).reshape(c.V + 1, 4) + np.uint64(7)
            for order in (orders if lanes is not None else orders[:1]):
                buf = zk.DeviceBuffer(start.nbytes)
                buf.upload(start)
                with lane_order(order):
                    bad = plan.solve(buf.ptr, k)
                got = buf.download(start.shape)
                buf.free()
                where = (name, "tape" if lanes is None else lanes, k, order)
                wrong = np.argwhere((got[:k] != expect_all[:k]).any(axis=2))
                assert wrong.size == 0, (where, "first wrong (row, column)", wrong[0].tolist(), "of", len(wrong))
                assert np.array_equal(got[k], start[k]), (where, "the sentinel row was written")
                assert bad == sum(bads[:k]), (where, bad, sum(bads[:k]))
        plan.close()


def check_program(zk, name, lanes_list, n_rows=2):
    """the compiled program of the wide plan at every lanes keeps the pass contract and, run over Python integers, gives the reference's rows
    and count"""
    c = cases.case(name)
    rows = cases.rows(name, n_rows)
    r = r1cs_of(c)
    for lanes in lanes_list:
        plan = make_plan(zk, c, lanes, r)
        records, coefs = plan.probe_program()
        info = plan.info()
        plan.close()
        assert records.shape == (info["records_or_passes"] + 1, prog.WORDS, lanes)
        passes = prog.decode(records)
        try:
            prog.check(passes, lanes, c.V, c.supplied, len(coefs))
            prog.check_bit_hints(passes, lanes, [(f, n) for k, _, f, n in c.hints if k == ref.BITS])
        except AssertionError as e:
            raise AssertionError((name, lanes) + e.args) from None
        for start, full, bad in rows:
            got, got_bad = prog.run(passes, coefs, start)
            wrong = [v for v in range(c.V + 1) if got[v] != full[v]]
            assert not wrong, (name, lanes, "first wrong column", wrong[0], "of", len(wrong))
            assert got_bad == bad, (name, lanes, got_bad, bad)


def message(zk, fn):
    with pytest.raises(zk.ZkError) as e:
        fn()
    return e.value.code, str(e.value)


def check_probe_arguments(zk):
    import ctypes as C
    c = cases.case("row_length_9")
    tape, wide = make_plan(zk, c, None), make_plan(zk, c, 8)
    n = C.c_size_t(0)
    buf = np.zeros(1 << 16, dtype=np.uint32)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    assert zk._lib.zk_wplan_probe_program(tape._h, p, C.c_size_t(buf.size), C.byref(n)) == 1          # ZK_ERR_ARG: a tape plan
    assert zk._lib.zk_wplan_probe_program(None, p, C.c_size_t(buf.size), C.byref(n)) == 1
    assert zk._lib.zk_wplan_probe_program(wide._h, p, C.c_size_t(buf.size), None) == 1
    assert zk._lib.zk_wplan_probe_program(wide._h, p, C.c_size_t(buf.size), C.byref(n)) == 0
    full = n.value
    assert full > (wide.info()["records_or_passes"] + 1) * prog.WORDS * 8 and (full - (wide.info()["records_or_passes"] + 1) * prog.WORDS * 8) % 8 == 0
    buf[:] = 0xdeadbeef
    assert zk._lib.zk_wplan_probe_program(wide._h, p, C.c_size_t(full - 1), C.byref(n)) == 1         # a short buffer: nothing is copied
    assert n.value == full and (buf == 0xdeadbeef).all()
    with pytest.raises(zk.ZkError):
        tape.probe_program()
    tape.close(); wide.close()


# ---------------------------------------------------------------- malformed variants of a generated system
def first_definitions(c):
    """{constraint: its target} by first appearance: a column that is neither supplied nor hinted and is first met in a C row"""
    hinted = {f + i for _, _, f, n in c.hints for i in range(n)}
    seen = set(c.supplied) | hinted
    out = {}
    for j, (ra, rb, rc) in enumerate(zip(c.rows_a, c.rows_b, c.rows_c)):
        for col, _ in rc:
            if col not in seen:
                out[j] = col
                seen.add(col)
    return out


def malformed(name):
    """{what is wrong: (the case, a word of the refusal)}"""
    c = cases.case(name)
    defs = first_definitions(c)
    j = sorted(defs)[len(defs) // 2]
    late = defs[sorted(defs)[-1]]
    copy = lambda rows: [list(r) for r in rows]
    out = {}
    rc = copy(c.rows_c); rc[j] = [(col, 0 if col == defs[j] else k) for col, k in rc[j]]
    out["target coefficient 0"] = (c._replace(rows_c=rc), "zero coefficient")
    rc = copy(c.rows_c); rc[j].append((late, 1))
    out["two unknowns in C"] = (c._replace(rows_c=rc), "introduces two new variables")
    ra = copy(c.rows_a); ra[j].insert(len(ra[j]) // 2, (late, 1))
    out["read before definition in A"] = (c._replace(rows_a=ra), "in A before anything defines it")
    rb = copy(c.rows_b); rb[j].append((late, 0))
    out["read before definition in B"] = (c._replace(rows_b=rb), "in B before anything defines it")
    for q, field in enumerate(("rows_a", "rows_b", "rows_c")):
        rows = copy(getattr(c, field)); rows[j].append((c.V + 1, 1))
        out["column above V in " + "ABC"[q]] = (c._replace(**{field: rows}), "exceeds the number of variables")
    free = [v for v in c.supplied if v]
    out["hint on a supplied variable"] = (c._replace(hints=c.hints + [(ref.INV, free[0], free[-1], 1)]), "supplied or defined twice")
    out["hint defines a variable twice"] = (c._replace(hints=c.hints + [(ref.INV, free[0], late, 1), (ref.NONZERO, free[0], late, 1)]), "supplied or defined twice")
    out["hint out of range"] = (c._replace(hints=c.hints + [(ref.BITS, free[0], c.V - 1, 3)]), "out of range")
    out["hint source out of range"] = (c._replace(hints=c.hints + [(ref.INV, c.V + 1, late, 1)]), "out of range")
    out["hint with first == 0"] = (c._replace(hints=c.hints + [(ref.BITS, free[0], 0, 1)]), "out of range")
    return out


def check_malformed(zk, name, lanes_list):
    for what, (c, word) in malformed(name).items():
        refused = message(zk, lambda: make_plan(zk, c, None))
        assert refused[0] == 1 and word in refused[1], (what, refused)
        for lanes in lanes_list:
            assert message(zk, lambda: make_plan(zk, c, lanes)) == refused, (what, lanes)
