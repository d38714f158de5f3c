"""Baby JubJub on the CPU emulation build of the HIP sources (csrc/jubjub.hpp, jubjub.cpp): the curve, hash-to-point, the Pedersen hash and
the three EdDSA schemes against the restatement of jubjub_cases.py and the pinned values of tests/golden/jubjub_kats.json; every error case with
its outputs proven untouched.  Everything is integer arithmetic and compares exactly.  test_jubjub_gpu.py runs the same checks on the device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from ethsnarks_amd import fields as F
import jubjub_cases as JC
import jubjub_checks as chk


@pytest.fixture(scope="module")
def emul_jubjub(emul):
    from conftest import ROOT
    d = os.path.join(ROOT, "tests", "emul_jubjub")
    so = os.path.join(d, "libzkhip_emul_jubjub.so")
    csrc = os.path.join(ROOT, "ethsnarks_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith("pp")] + [emul, os.path.join(d, "Makefile")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", d, "-s"])
    return so


@pytest.fixture(scope="module")
def zk(emul_jubjub):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul_jubjub)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    prover._lib = None
    prover._lib_path_loaded = None


@pytest.fixture(scope="module")
def J(zk):
    from ethsnarks_amd import jubjub
    jubjub._lib()
    return jubjub


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


def code(zk, fn, *a, **kw):
    with pytest.raises(zk.ZkError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------- pinned values
def test_constants_and_pinned_values(J):
    chk.check_constants(J)
    chk.check_kats(J)


def test_hash_to_point_and_basepoints(J):
    chk.check_hash_to_point(J)


# ---------------------------------------------------------------- the curve
def test_point_operations(J):
    chk.check_point_ops(J, 20)


def test_scalar_multiplication(J):
    chk.check_scalar_mul(J, 20)


# ---------------------------------------------------------------- Pedersen
def test_pedersen_windows(J):
    chk.check_pedersen(J)


def test_pedersen_tables(J):
    chk.check_tables(J)


# ---------------------------------------------------------------- EdDSA
@pytest.mark.parametrize("scheme", chk.SCHEMES)
def test_signatures(J, scheme):
    chk.check_signatures(J, scheme)


def test_cross_scheme(J):
    chk.check_cross_scheme(J)


@pytest.mark.parametrize("scheme", chk.SCHEMES)
def test_batch_parity(J, scheme):
    A, sigs, msgs, want = JC.batch(scheme, 3, 70)                      # more than a workgroup; the device test runs 130
    with J.EdDSAVerifier(scheme, msg_len=3) as v:
        assert v.verify(A, sigs, msgs) == want


# ---------------------------------------------------------------- errors: ZK_ERR_ARG (1) and nothing written
TOP = (1 << 256) - 1
G8 = F.ints_to_limbs(list(JC.GENERATOR)).reshape(1, 8)


def pts(*points):
    return F.ints_to_limbs([c for p in points for c in p]).reshape(-1, 8)


def test_curve_errors(zk, J):
    L = zk._lib
    good, off = JC.GENERATOR, JC.OFF_CURVE
    for bad in ((JC.Q, 1), (0, JC.Q), (TOP, 1), off):
        for pos in (0, 2):                                             # the first and the last item
            p = [good] * 3
            p[pos] = bad
            out = np.full((3, 8), 7, dtype=np.uint64)
            for op in (0, 1, 2):
                assert L.zk_jj_point_op(op, zk._p64(pts(*p)), zk._p64(pts(*[good] * 3)), C.c_uint32(3), 0, zk._p64(out)) == 1, (bad, op)
                assert (out == 7).all()
            assert L.zk_jj_point_op(0, zk._p64(pts(*[good] * 3)), zk._p64(pts(*p)), C.c_uint32(3), 0, zk._p64(out)) == 1 and (out == 7).all()
            assert L.zk_jj_scalar_mul(zk._p64(pts(*p)), zk._p64(F.ints_to_limbs([1, 2, 3])), C.c_uint32(3), 0, zk._p64(out)) == 1 and (out == 7).all()
    out = np.full((1, 8), 7, dtype=np.uint64)
    assert L.zk_jj_point_op(3, zk._p64(G8), zk._p64(G8), C.c_uint32(1), 0, zk._p64(out)) == 1 and (out == 7).all()
    assert L.zk_jj_point_op(0, zk._p64(G8), None, C.c_uint32(1), 0, zk._p64(out)) == 1 and (out == 7).all()
    assert L.zk_jj_point_op(1, None, None, C.c_uint32(1), 0, zk._p64(out)) == 1
    assert L.zk_jj_scalar_mul(None, None, C.c_uint32(1), 0, None) == 1
    assert code(zk, J.point_add, [off], [good]) == 1 and code(zk, J.scalar_mul, [off], [5]) == 1
    assert J.point_add([], []) == [] and J.scalar_mul([], []) == []


def test_name_and_index_errors(zk, J):
    out = np.full(8, 7, dtype=np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert zk._lib.zk_jj_pedersen_basepoint(b"x" * 29, 0, p) == 1 and (out == 7).all()
    assert zk._lib.zk_jj_pedersen_basepoint(b"x", 0x10000, p) == 1 and (out == 7).all()
    assert zk._lib.zk_jj_pedersen_basepoint(None, 0, p) == 1 and zk._lib.zk_jj_hash_to_point(None, 3, p) == 1 and (out == 7).all()
    assert code(zk, J.PedersenHasher, b"x" * 29, 30) == 1
    assert code(zk, J.PedersenHasher, b"x", 0) == 1 and code(zk, J.PedersenHasher, b"x", 3 * 62 * 256 + 1) == 1
    assert J.pedersen_basepoint(b"x" * 28, 0xFFFF) == JC.basepoint(b"x" * 28, 0xFFFF)


def test_pedersen_errors(zk, J):
    with J.PedersenHasher(b"test", 3 * 10) as h:
        def call(win, counts, stride, n):
            out = np.full((n, 8), 7, dtype=np.uint64)
            w = np.array(win, dtype=np.uint8)
            c = np.array(counts, dtype=np.uint32) if counts is not None else None
            rc = zk._lib.zk_pedersen_hash(h._h, w.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p) if c is not None else None, stride, n, out.ctypes.data_as(C.c_void_p))
            assert (out == 7).all() or rc == 0
            return rc
        assert call([[1, 2, 3], [4, 5, 6]], [3, 2], 3, 2) == 0
        assert call([[1, 2, 3], [4, 8, 6]], [3, 2], 3, 2) == 1         # a window > 7, in the second row
        assert call([[1, 2, 3], [4, 5, 255]], None, 3, 2) == 1
        assert call([[1, 2, 3], [4, 5, 6]], [3, 0], 3, 2) == 1         # a count of 0
        assert call([[1, 2, 3], [4, 5, 6]], [4, 1], 3, 2) == 1         # above the stride
        assert call([[0] * 11], [11], 11, 1) == 1                      # above the capacity
        assert call([[0] * 11], None, 11, 1) == 1
        assert call([[0] * 11], [10], 11, 1) == 0
        assert call([[1]], None, 0, 1) == 1
        assert code(zk, h.hash_windows, [[1, 2], [9]]) == 1 and code(zk, h.hash_windows, [[1], []]) == 1
        assert code(zk, h.table, 5, 6) == 1 and len(h.table(5, 5)) == 5
        assert h.hash_windows([]) == []


def test_eddsa_errors(zk, J):
    L = zk._lib
    h = C.c_void_p(1)
    for scheme, B, msg_len in ((3, None, 1), (-1, None, 1), (0, None, 0), (1, None, 4097), (1, pts(JC.OFF_CURVE), 1), (1, pts((JC.Q, 1)), 1)):
        h.value = 1
        assert L.zk_eddsa_create(scheme, B.ctypes.data_as(C.c_void_p) if B is not None else None, msg_len, 0, C.byref(h)) == 1 and not h.value
    assert code(zk, J.EdDSAVerifier, "pure", B=JC.OFF_CURVE, msg_len=1) == 1
    good = chk.sig_cases("mimc", 1)[0]
    with J.EdDSAVerifier("mimc", msg_len=1) as v:
        for bad_item in (1, 2):                                        # the last of two or three items
            n = bad_item + 1
            for field in ("Ax", "Ry", "s", "m"):
                for bad in (JC.Q, TOP):
                    A = [list(good[1]) for _ in range(n)]; R = [list(good[2][0]) for _ in range(n)]; s = [good[2][1]] * n; m = [list(good[3]) for _ in range(n)]
                    if field == "Ax": A[bad_item][0] = bad
                    if field == "Ry": R[bad_item][1] = bad
                    if field == "s": s[bad_item] = bad
                    if field == "m": m[bad_item][0] = bad
                    out = np.full(n, 7, dtype=np.uint8)
                    arrs = [pts(*A), pts(*R), F.ints_to_limbs(s), F.ints_to_limbs([x for r in m for x in r])]
                    rc = L.zk_eddsa_verify_batch(v._h, *[a.ctypes.data_as(C.c_void_p) for a in arrs], n, out.ctypes.data_as(C.c_void_p))
                    assert rc == 1 and (out == 7).all(), (field, bad_item)
        assert L.zk_eddsa_verify_batch(v._h, None, None, None, None, 1, None) == 1
        assert v.verify([], [], []) == []
    with J.EdDSAVerifier("pure", msg_len=2) as v:                      # the s check holds for the byte schemes too
        c = chk.sig_cases("pure", 3)[0]
        assert code(zk, v.verify, [c[1]], [(c[2][0], JC.Q)], [b"ab"]) == 1
