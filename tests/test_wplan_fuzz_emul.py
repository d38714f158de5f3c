"""Both witness plans on the CPU emulation build of the HIP sources against the big-int solver of wplan_ref.py: the directed systems of
wplan_cases.py (row lengths, operand shapes, row reuse, pass splitting, slot pressure with eviction, the refused level, hints) and the
generated systems seed_0 .. seed_{N-1}, on the tape plan and on the wide plan at lanes 4, 8, 16, 32 and 64, the wide solves in both lane
orders of the stand-in (a result that depends on the order in which the lanes of a pass run differs from the reference in one of them);
the compiled program of every wide plan decoded, checked against the pass contract and interpreted (wplan_program.py); the refusals of
malformed variants.  N = 24 generated systems; the module takes about 55 s on one core.  test_wplan_fuzz_gpu.py runs the same checks on
the device."""
import ctypes as C
import pytest
import wplan_cases as cases
import wplan_fuzz_checks as chk

N_SEEDS = 24
NAMES = sorted(cases.DIRECTED) + ["seed_%d" % s for s in range(N_SEEDS)]
N_ROWS = 64 // 4 + 1
ORDERS = ("ascending", "reverse")


@pytest.fixture(scope="module")
def zk(emul):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul)
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
    return (1, 64 // (lanes or 64) + 1)                              # a lone witness; a second workgroup starts (the tape: 64 lanes, 64 witnesses)


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_counts_are_the_references(zk, name):
    chk.check_solves(zk, name, chk.PLANS, ks_for, N_ROWS, ORDERS)


@pytest.mark.parametrize("name", NAMES)
def test_program_keeps_the_pass_contract(zk, name):
    chk.check_program(zk, name, cases.LANES)


def test_tape_fills_a_whole_wave_and_one_more(zk):
    chk.check_solves(zk, "seed_0", (None,), lambda lanes: (65,), 65)


@pytest.mark.parametrize("name", sorted(cases.REUSE))
def test_a_repeated_row_is_evaluated_once_within_the_reuse_distance(zk, name):
    """distance 32 (WW_REUSE) still reuses the temporary, 33 does not, a changed coefficient is another row: the number of DOTs says which"""
    for lanes in cases.LANES:
        plan = chk.make_plan(zk, cases.case(name), lanes)
        assert plan.info()["dots"] == cases.expected_dots(name), (name, lanes)
        plan.close()


@pytest.mark.parametrize("name", ["slot_pressure_forward", "slot_pressure_reverse"])
def test_slot_pressure_saturates_the_pool_at_4_lanes(zk, name):
    """128 slots at 4 lanes, all of them in use at the peak: variables lose their slots to temporaries and are read from the witness row"""
    plan = chk.make_plan(zk, cases.case(name), 4)
    assert plan.info()["lds_slots"] == 128
    plan.close()
    for lanes in (8, 16):                                            # nothing is evicted: the 160 products, and what the chain holds
        plan = chk.make_plan(zk, cases.case(name), lanes)
        assert plan.info()["lds_slots"] == 164
        plan.close()


def test_a_level_of_320_temporaries_is_refused_at_4_and_8_lanes(zk):
    """the documented limit: temporaries cannot leave LDS.  The tape and 64 lanes accept the system and solve it."""
    c = cases.case("refused_level")
    for lanes in (4, 8):
        code, text = chk.message(zk, lambda: chk.make_plan(zk, c, lanes))
        assert code == 1 and "live LDS slots" in text, (lanes, text)
    chk.check_solves(zk, "refused_level", (None, 64), ks_for, 3, ORDERS)
    chk.check_program(zk, "refused_level", (64,))


@pytest.mark.parametrize("name", ["seed_0", "seed_1"])
def test_malformed_variants_are_refused_alike(zk, name):
    chk.check_malformed(zk, name, (4, 16, 64))


def test_probe_arguments(zk):
    chk.check_probe_arguments(zk)
