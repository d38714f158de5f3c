"""Both witness plans on the device (k_witness_tape, k_witness_wide at lanes 4, 8, 16, 32 and 64) against the big-int solver of wplan_ref.py:
the directed systems of wplan_cases.py and a handful of generated ones, k = 1, 5 and 67 witnesses per call; the program of a few wide plans
read back from device memory (zk_wplan_probe_program), checked against the pass contract and interpreted; the refusals of malformed
variants.  test_wplan_fuzz_emul.py documents the checks.  Every system is a few hundred constraints: a test takes seconds."""
import pytest
import wplan_cases as cases
import wplan_fuzz_checks as chk

pytestmark = pytest.mark.gpu

NAMES = sorted(cases.DIRECTED) + ["seed_%d" % s for s in range(4)]
KS = (1, 5, 67)                                                       # a lone witness; a partly filled wave; more than one workgroup at every lanes


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_counts_are_the_references(hip, name):
    chk.check_solves(hip, name, chk.PLANS, lambda lanes: KS, max(KS))


@pytest.mark.parametrize("name", ["row_length_513", "slot_pressure_reverse", "seed_0"])
def test_program_read_back_keeps_the_pass_contract(hip, name):
    chk.check_program(hip, name, (4, 16, 64))


def test_a_level_of_320_temporaries_is_refused_at_4_and_8_lanes(hip):
    c = cases.case("refused_level")
    for lanes in (4, 8):
        code, text = chk.message(hip, lambda: chk.make_plan(hip, c, lanes))
        assert code == 1 and "live LDS slots" in text, (lanes, text)
    chk.check_solves(hip, "refused_level", (None, 64), lambda lanes: KS, max(KS))


def test_malformed_variants_are_refused_alike(hip):
    chk.check_malformed(hip, "seed_0", (4, 16, 64))


def test_probe_arguments(hip):
    chk.check_probe_arguments(hip)
