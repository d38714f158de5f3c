"""The bucket sort of the multi-scalar multiplications on the device: zk_msm_sort_probe bucket by bucket against Python integers on the cases
of msmsort_cases.py (every window width 2 .. 20 on the edge scalars of its recoding, the direct scatter, the sort shapes), the probe's
refusals, and the multi-exponentiation of the edge scalars against the oracle at every width (G1) and at five widths (G2).
test_msmsort_emul.py and msmsort_checks.py document the checks.  At most a few thousand scalars and about a hundred distinct bases: a test
takes a fraction of a second, most of it in the Python reference, which is computed once per case."""
import pytest
import msmsort_cases as cases
import msmsort_checks as chk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.WIDTH_CASES)
def test_sort_of_edge_scalars_at_every_width(hip, monkeypatch, name):
    chk.check_sort(hip, name, monkeypatch)


@pytest.mark.parametrize("name", cases.DIRECT_CASES)
def test_direct_scatter_at_every_width(hip, monkeypatch, name):
    chk.check_sort(hip, name, monkeypatch)


@pytest.mark.parametrize("name", cases.SHAPE_CASES)
def test_sort_shapes(hip, monkeypatch, name):
    chk.check_sort(hip, name, monkeypatch)


def test_probe_refusals(hip, monkeypatch):
    chk.check_refusals(hip, monkeypatch)


@pytest.mark.parametrize("c", cases.MSM_G1_WIDTHS)
def test_msm_g1_of_edge_scalars_at_every_width(hip, oracle, monkeypatch, c):
    chk.check_msm(hip, oracle, c, False, monkeypatch)


@pytest.mark.parametrize("c", cases.MSM_G2_WIDTHS)
def test_msm_g2_of_edge_scalars(hip, oracle, monkeypatch, c):
    chk.check_msm(hip, oracle, c, True, monkeypatch)
