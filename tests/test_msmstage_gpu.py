"""The stages of the multi-scalar multiplications behind the bucket sort, on the device: zk_msm_stage_probe -- the table of window multiples,
the chunk pieces, the heavy list, the bucket sums, the row / column sums, the weighted sum and the folded result -- value by value against
Python integers on the cases of msmstage_cases.py (all but the ones that exist for the emulation build's small slot count).
msmstage_checks.py documents the checks and test_msmstage_emul.py runs the same ones on the CPU emulation build.

On a device every case takes ChunkRule::len's first branch, seg = seg_min = 8 (the only one a device reaches below about 2 M entries):
the cases assert that from the slots the probe reports.

Measured on an MI355X: 137 tests in 18.8 s.  The corner cases at c = 20 take 0.9 - 1.0 s each (2^20 buckets of two planes copied back and
checked in bulk), the refusals 0.8 s, the c = 17 corner cases and the sparse c = 20 cases about 0.5 s, everything else under 0.3 s."""
import pytest
import msmstage_cases as cases
import msmstage_checks as chk

pytestmark = pytest.mark.gpu
_ON_DEVICE = lambda names: [n for n in names if n in cases.DEVICE_CASES]


@pytest.mark.parametrize("name", _ON_DEVICE(cases.TABLE_CASES))
def test_table_of_window_multiples(hip, oracle, monkeypatch, name):
    chk.check_case(hip, oracle, name, monkeypatch, False)


@pytest.mark.parametrize("name", _ON_DEVICE(cases.ACC_CASES))
def test_chunk_pieces(hip, oracle, monkeypatch, name):
    """seg = seg_min = 8 throughout: the only branch of ChunkRule::len a real device reaches below about 2 M entries"""
    chk.check_case(hip, oracle, name, monkeypatch, False)


@pytest.mark.parametrize("name", _ON_DEVICE(cases.HEAVY_CASES))
def test_bucket_sums_and_heavy_list(hip, oracle, monkeypatch, name):
    chk.check_case(hip, oracle, name, monkeypatch, False)


@pytest.mark.parametrize("name", _ON_DEVICE(cases.TAIL_CASES))
def test_row_column_and_weighted_sums(hip, oracle, monkeypatch, name):
    chk.check_case(hip, oracle, name, monkeypatch, False)


def test_probe_refusals(hip, oracle, monkeypatch):
    chk.check_refusals(hip, oracle, monkeypatch, False)
