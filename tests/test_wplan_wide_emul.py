"""The wide (lane-parallel) witness plan on the CPU emulation build of the HIP sources (csrc/wplan_wide.hpp: the plan compiler and
k_witness_wide, whose lanes run as fibers that yield at __syncthreads()): parity with the tape plan and the front end, the violation
counts, the hints, the refusals, the schedule of hand-made systems whose answer can be derived, and the chain through to a proof.
test_wplan_wide_gpu.py runs the parity, violation and hint checks on the device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F, r1cs as R
import merkle_cases as MC
import poseidon_cases as PC
import wplan_wide_checks as chk


@pytest.fixture(scope="module")
def emul_merkle(emul):
    from conftest import ROOT
    d = os.path.join(ROOT, "tests", "emul_merkle")
    so = os.path.join(d, "libzkhip_emul_merkle.so")
    csrc = os.path.join(ROOT, "ethsnarks_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith("pp")] + [emul, os.path.join(d, "Makefile")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", d, "-s"])
    return so


@pytest.fixture(scope="module")
def zk(emul_merkle):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul_merkle)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    prover._lib = None
    prover._lib_path_loaded = None


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


def ks_for(lanes):
    return (1, 64 // lanes + 1)                                      # a partly filled wave; a second workgroup starts


# ---------------------------------------------------------------- 1, 2: parity with the tape and the front end; the checks count the same
@pytest.mark.parametrize("lanes", [4, 16, 64])
@pytest.mark.parametrize("name", chk.CASES)
def test_rows_are_the_tapes_and_the_front_ends(zk, name, lanes):
    chk.check_parity(zk, name, lanes, ks_for(lanes))


@pytest.mark.parametrize("lanes", [4, 16, 64])
@pytest.mark.parametrize("name", chk.CASES)
def test_checks_count_what_the_tape_counts(zk, name, lanes):
    chk.check_violations(zk, name, lanes, ks_for(lanes))


# ---------------------------------------------------------------- 3: hints
def test_bit_hints(zk):
    chk.check_bit_hints(zk, 16)


def test_inverse_and_nonzero_hints(zk):
    chk.check_inv_nonzero_hints(zk, 16)


# ---------------------------------------------------------------- 4: refusals
def system(rows_a, rows_b, rows_c, V):
    return R.R1CS(len(rows_a), 1, V, R.CSR.from_rows(rows_a), R.CSR.from_rows(rows_b), R.CSR.from_rows(rows_c))


def test_refusals_are_the_tapes(zk):
    r, supplied, _ = chk.case("mimc_preimage")
    a = chk.message(zk, lambda: zk.WitnessPlan(r, supplied[:-1]))              # a message word neither supplied nor defined
    b = chk.message(zk, lambda: zk.WitnessPlan(r, supplied[:-1], lanes=16))
    assert a == b and a[0] == 1 and "before anything defines it" in a[1]
    two = system([[(1, 1)]], [[(1, 1)]], [[(2, 1), (3, 1)]], 3)                # w1 w1 = w2 + w3
    a = chk.message(zk, lambda: zk.WitnessPlan(two, [0, 1]))
    b = chk.message(zk, lambda: zk.WitnessPlan(two, [0, 1], lanes=16))
    assert a == b and a[0] == 1 and "introduces two new variables (2 and 3)" in a[1]
    lonely = system([[(1, 1)]], [[(1, 1)]], [[(2, 1)]], 3)                     # nothing defines w3
    a = chk.message(zk, lambda: zk.WitnessPlan(lonely, [0, 1]))
    b = chk.message(zk, lambda: zk.WitnessPlan(lonely, [0, 1], lanes=16))
    assert a == b and a[0] == 1 and "neither supplied nor defined" in a[1]
    for lanes in (0, 3, 2, 128):
        code, _ = chk.message(zk, lambda: zk.WitnessPlan(r, supplied, lanes=lanes))
        assert code == 1, lanes


# ---------------------------------------------------------------- 5: the schedule
def test_schedule_of_independent_constraints(zk):
    n = 40                                                                     # w[n + i] = w[i] w[i], i = 1 .. n: one level, ceil(40 / 16) passes
    r = system([[(i, 1)] for i in range(1, n + 1)], [[(i, 1)] for i in range(1, n + 1)], [[(n + i, 1)] for i in range(1, n + 1)], 2 * n)
    plan = zk.WitnessPlan(r, list(range(0, n + 1)), lanes=16)
    info = plan.info()
    assert info["levels"] == 1 and info["records_or_passes"] == 3 and info["steps"] == 40 and info["dots"] == 0 and info["max_level_ops"] == 40
    assert info["products"] == 40
    plan.close()


def test_schedule_of_a_chain(zk):
    n = 40                                                                     # w[i + 1] = w[i] w[i]: nothing to spread
    r = system([[(i, 1)] for i in range(1, n + 1)], [[(i, 1)] for i in range(1, n + 1)], [[(i + 1, 1)] for i in range(1, n + 1)], n + 1)
    plan = zk.WitnessPlan(r, [0, 1], lanes=16)
    info = plan.info()
    assert info["levels"] == 40 and info["records_or_passes"] == 40 and info["max_level_ops"] == 1
    plan.close()


def test_schedule_of_a_long_row_and_its_reuse(zk):
    """a 64-term combination with general coefficients, T = 8: eight chunk DOTs (level 1), the DOT over their temporaries (level 2), the STEP
    (level 3).  The same row as A and as B is evaluated once.  The values are the tape's."""
    n = 64
    row = [(i, i + 2) for i in range(1, n + 1)]
    for rows_b in ([[(0, 1)]], [row]):
        r = system([row], rows_b, [[(n + 1, 1)]], n + 1)
        supplied = list(range(0, n + 1))
        tape, wide = zk.WitnessPlan(r, supplied), zk.WitnessPlan(r, supplied, lanes=16)
        info = wide.info()
        assert info["dots"] == 9 and info["levels"] == 3 and info["steps"] == 1 and info["ops"] == 10
        assert info["products"] == 64 + 1                                      # the coefficient products once, and a x b
        assert tape.info()["products"] == 64 * (2 if rows_b == [row] else 1) + 1
        start = np.zeros((3, r.V + 1, 4), dtype=np.uint64)
        start[:2, :n + 1] = F.fr_to_mont([1] + [3 * i + 1 for i in range(n)])
        start[2] = 9
        (bad_t, got_t), (bad_w, got_w) = chk.solve_both(zk, tape, wide, start, 2)
        assert bad_t == 0 and bad_w == 0 and np.array_equal(got_w, got_t)
        s = sum((i + 2) * (3 * (i - 1) + 1) for i in range(1, n + 1))
        assert np.array_equal(got_w[0, n + 1], F.fr_to_mont([s * s if rows_b == [row] else s])[0])
        tape.close(); wide.close()


def test_schedule_of_the_poseidon_preimage_circuit(zk):
    r, supplied, _ = chk.case("poseidon_preimage")
    assert r.nC == 317
    one, minus_one = F.fr_to_mont([1])[0], F.fr_to_mont([-1 % G.FR])[0]
    tape_products = 0                                                          # the tape's kind-2 terms: a general coefficient on a variable
    for m in (r.A, r.B, r.C):
        general = (m.col != 0) & ~(m.coeff == one).all(axis=1) & ~(m.coeff == minus_one).all(axis=1) & (m.coeff != 0).any(axis=1)
        tape_products += int(general.sum())
    tape, wide = zk.WitnessPlan(r, supplied), zk.WitnessPlan(r, supplied, lanes=16)
    ti, wi = tape.info(), wide.info()
    assert ti["kind"] == 0 and ti["lanes"] == 0 and ti["levels"] == 0 and ti["records_or_passes"] > r.nC
    assert wi["products"] < tape_products / 2
    assert wi["levels"] < ti["records_or_passes"]
    assert wi["steps"] == r.nC and wi["ops"] == wi["dots"] + wi["steps"] and wi["lds_slots"] <= 32 * 16
    tape.close(); wide.close()


def test_a_system_that_does_not_fit_its_lds_share_is_refused(zk):
    """200 long rows whose readers all wait for one late variable: 200 temporaries are live at once, a group of 4 lanes has 128 slots"""
    m, n = 200, 9
    chain = 4                                                                  # w2 = w1 w1, w3 = w2 w2, ...: the late variable is w[chain + 1]
    late, base = chain + 1, chain + 2
    a = [[(i, 1)] for i in range(1, chain + 1)] + [[(base + (i + t) % 16, 3 + i + t) for t in range(n)] for i in range(m)]
    b = [[(i, 1)] for i in range(1, chain + 1)] + [[(late, 1)]] * m
    c = [[(i + 1, 1)] for i in range(1, chain + 1)] + [[(base + 16 + i, 1)] for i in range(m)]
    r = system(a, b, c, base + 16 + m - 1)
    supplied = [0, 1] + list(range(base, base + 16))
    code, text = chk.message(zk, lambda: zk.WitnessPlan(r, supplied, lanes=4))
    assert code == 1 and "live LDS slots" in text and "level" in text
    zk.WitnessPlan(r, supplied, lanes=16).close()                              # 512 slots: fits


# ---------------------------------------------------------------- 6: through to a proof
def test_membership_chain_depth_3_with_the_wide_plan(zk, oracle):
    from ethsnarks_amd import merkle as M
    D, n = 3, 7
    leaves = MC.random_leaves(n, 950)
    ref = PC.PyTree(D, 2, leaves)
    t = M.MerkleTree(2 ** D, width=2, hasher="poseidon")
    t.extend(leaves)
    indices = [0, 6, 3]
    cases = [G.poseidon_membership_circuit(D, leaf=leaves[i], address=i, path=ref.path(i)) for i in indices]
    r = cases[0][0]
    k = len(indices)
    supplied = list(range(0, 1 + 1 + D + D + 1))
    sentinel = np.arange(4 * (r.V + 1) * (k + 1), dtype=np.uint64).reshape(k + 1, r.V + 1, 4) + np.uint64(7)
    buf = zk.DeviceBuffer(32 * (r.V + 1) * (k + 1))
    buf.upload(sentinel)
    t.fill_witnesses(indices, buf, r)
    plan = zk.WitnessPlan(r, supplied, lanes=16)
    assert plan.solve(buf.ptr, k) == 0
    got = buf.download((k + 1, r.V + 1, 4))
    for p in range(k):
        assert np.array_equal(got[p], F.fr_to_mont(cases[p][1])), p
    assert np.array_equal(got[k], sentinel[k])
    pk, vk = zk.keygen(r, seed=33)
    ctx = zk.ProverContext(pk, r)
    text = zk.prove(ctx, got[1])
    assert text == oracle.prove(oracle.pk_from_parts(pk.parts()), r, F.fr_to_mont(cases[1][1]))[0]
    assert zk.stub_verify(vk.to_json(), text)
    ctx.close(); plan.close(); buf.free()
