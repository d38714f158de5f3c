"""The witness fill of the MiMC-EdDSA circuit with 2 and 4 lanes per signature (csrc/jubjub.hpp k_eddsa_fill_wide, zk_eddsa_fill_witnesses_wide)
on the CPU emulation build of the HIP sources, whose workgroups run as fibers that yield at every barrier: rows against the front end's witness
at n = 1 (one live witness in a workgroup), 3 (valid, wrong, off-curve side by side) and 65 (a tail workgroup with one live witness, malformed
items between full rows), a workgroup without a live witness, three message elements, the descending lane order, the bytes of the one-lane
fill, and the refusals.  test_eddsa_wide_gpu.py runs the same checks on the device."""
import ctypes as C

import pytest

import eddsa_circuit_cases as EC
import eddsa_wide_checks as chk
import jubjub_cases as JC
from test_jubjub_emul import emul_jubjub, zk, J                        # noqa: F401  (the fixtures that build and load the emulation library)


@pytest.fixture(autouse=True)
def no_guard_violations(zk):
    zk._lib.zk_emul_guard_violations.restype = C.c_uint64
    yield
    bad = int(zk._lib.zk_emul_guard_violations())
    assert bad == 0, "%d device buffers were written past their end" % bad


@pytest.mark.parametrize("n", EC.SIZES)
@pytest.mark.parametrize("lanes", chk.WIDE)
def test_rows_and_verdicts(zk, J, lanes, n):
    chk.check_rows(zk, J, n, lanes)


@pytest.mark.parametrize("lanes", chk.WIDE)
def test_a_workgroup_without_a_live_witness(zk, J, lanes):
    chk.check_dead_workgroup(zk, J, lanes)


def test_three_message_elements_and_another_base_point(zk, J):
    chk.check_rows(zk, J, 3, 4, msg_len=3, B=JC.mul(JC.GENERATOR, 77))


def test_descending_lane_order_gives_the_same_rows(zk, J, monkeypatch):
    """every LDS slot and every row element is written in one barrier interval and read in a later one, so the order in which the emulator runs
    the lanes between two barriers (read from the environment at every launch) does not enter: the descending sweep leaves the rows that
    test_rows_and_verdicts[4-65] holds the ascending sweep to, element for element"""
    monkeypatch.setenv("ZK_EMUL_LANE_ORDER", "reverse")
    chk.check_rows(zk, J, 65, 4)


def test_same_bytes_as_one_lane(zk, J):
    chk.check_same_bytes_as_one_lane(zk, J)


def test_refusals(zk, J):
    chk.check_refusals(zk, J)
