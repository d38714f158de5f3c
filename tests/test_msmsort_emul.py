"""The bucket sort of the multi-scalar multiplications (msm_digit, k_sort_count, k_sort_colscan, k_sort_binscan, k_sort_partition,
k_sort_partition_staged, k_sort_fine; SortShape) on the CPU emulation build of the HIP sources: zk_msm_sort_probe bucket by bucket against
Python integers on the cases of msmsort_cases.py -- every window width 2 .. 20 on scalars built for the edges of its signed-digit recoding,
the direct scatter (ZK_SORT_PER_GROUP=1024), and the sort shapes the proving path reaches only by accident -- the probe's refusals, and
the multi-exponentiation of those scalars against the oracle at every width.  msmsort_checks.py documents the checks; test_msmsort_gpu.py
runs the same ones on the device.

Measured on the stand-in: a probe call costs 1.2 - 1.5 s whatever the scalars (k_sort_fine's 1024 fibers per coarse bin), a width case (two
calls) 2.2 - 2.6 s, a multi-exponentiation 1.5 - 5 s (G1) and 3 - 7 s (G2), the emulated reduction over 2^19 nearly empty buckets included:
nothing stands out against the other emulation tests, so nothing is marked slow."""
import ctypes as C
import pytest
import msmsort_cases as cases
import msmsort_checks as chk


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


@pytest.mark.parametrize("c", cases.WIDTHS)
def test_edge_scalars_reach_the_recoding_edges(c):
    cases.edge_scalars(c)                                            # asserts what the family is there for; CASES asserted its shapes on import


@pytest.mark.parametrize("name", cases.WIDTH_CASES)
def test_sort_of_edge_scalars_at_every_width(zk, monkeypatch, name):
    chk.check_sort(zk, name, monkeypatch)


@pytest.mark.parametrize("name", cases.DIRECT_CASES)
def test_direct_scatter_at_every_width(zk, monkeypatch, name):
    chk.check_sort(zk, name, monkeypatch)


@pytest.mark.parametrize("name", cases.SHAPE_CASES)
def test_sort_shapes(zk, monkeypatch, name):
    chk.check_sort(zk, name, monkeypatch)


def test_probe_refusals(zk, monkeypatch):
    chk.check_refusals(zk, monkeypatch)


@pytest.mark.parametrize("c", cases.MSM_G1_WIDTHS)
def test_msm_g1_of_edge_scalars_at_every_width(zk, oracle, monkeypatch, c):
    chk.check_msm(zk, oracle, c, False, monkeypatch)


@pytest.mark.parametrize("c", cases.MSM_G2_WIDTHS)
def test_msm_g2_of_edge_scalars(zk, oracle, monkeypatch, c):
    chk.check_msm(zk, oracle, c, True, monkeypatch)
