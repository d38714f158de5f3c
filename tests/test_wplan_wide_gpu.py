"""The wide (lane-parallel) witness plan on the device (csrc/wplan_wide.hpp, k_witness_wide): the parity, violation and hint checks of
test_wplan_wide_emul.py (wplan_wide_checks.py), and the depth-29 Poseidon membership circuit through to the proofs."""
import time
import numpy as np
import pytest
from ethsnarks_amd import gadgets as G, fields as F
import wplan_wide_checks as chk

pytestmark = pytest.mark.gpu

KS = (1, 5, 67)                                                       # a lone witness; a partly filled wave; more than one workgroup at every lanes


@pytest.mark.parametrize("lanes", [8, 16, 64])
@pytest.mark.parametrize("name", chk.CASES)
def test_rows_are_the_tapes_and_the_front_ends(hip, name, lanes):
    chk.check_parity(hip, name, lanes, KS)


@pytest.mark.parametrize("lanes", [8, 16, 64])
@pytest.mark.parametrize("name", chk.CASES)
def test_checks_count_what_the_tape_counts(hip, name, lanes):
    chk.check_violations(hip, name, lanes, KS)


def test_bit_hints(hip):
    chk.check_bit_hints(hip, 16)


def test_inverse_and_nonzero_hints(hip):
    chk.check_inv_nonzero_hints(hip, 16)


def test_poseidon_membership_depth_29(hip):
    """9 339 constraints, 63-term rows, a 300 KB row: the wide solve is byte-identical to the tape solve, and so are the proofs from the two
    buffers.  Prints both solve times; asserts none."""
    D, k, lanes = 29, 32, 16
    made = [G.poseidon_membership_circuit(D), G.poseidon_membership_circuit(D, leaf=4242, address=0x155aa55, path=[1000 + 3 * d for d in range(D)])]
    r = made[0][0]
    assert r.nC == 9339
    supplied = list(range(0, 1 + 1 + D + D + 1))
    ws = [F.fr_to_mont(m[1]) for m in made]
    start = np.zeros((k, r.V + 1, 4), dtype=np.uint64)
    for p in range(k):
        start[p, supplied] = ws[p % 2][supplied]
    tape, wide = hip.WitnessPlan(r, supplied), hip.WitnessPlan(r, supplied, lanes=lanes)
    print("tape %s\nwide %s" % (tape.info(), wide.info()))
    bufs, took = [], []
    for plan in (tape, wide):
        buf = hip.DeviceBuffer(start.nbytes)
        buf.upload(start)
        assert plan.solve(buf.ptr, k) == 0                              # (warm-up)
        buf.upload(start)
        t0 = time.perf_counter()
        assert plan.solve(buf.ptr, k) == 0
        took.append(1e3 * (time.perf_counter() - t0))
        bufs.append(buf)
    print("solve of %d witnesses: tape %.1f ms, wide (%d lanes) %.1f ms" % (k, took[0], lanes, took[1]))
    got_t, got_w = bufs[0].download(start.shape), bufs[1].download(start.shape)
    assert np.array_equal(got_w, got_t)
    for p in range(k):
        assert np.array_equal(got_w[p], ws[p % 2]), p
    pk, _ = hip.keygen(r, seed=31)
    ctx = hip.ProverContext(pk, r, max_batch=k)
    texts = []
    for buf, got in ((bufs[0], got_t), (bufs[1], got_w)):
        ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
        parts, _ = ctx.collect_batch(k)
        texts.append([hip.proof_to_json(ctx.prove_combine(parts[p]), got[p][1:2]) for p in range(k)])
    assert texts[1] == texts[0] and len(set(texts[1])) == 2
    ctx.close(); tape.close(); wide.close()
    for buf in bufs:
        buf.free()
