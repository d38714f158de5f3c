"""The stages of the multi-scalar multiplications behind the bucket sort (k_msm_precompute, k_msm_accumulate, k_msm_bucket_finalize,
k_msm_heavy, k_msm_rowcol_sum, k_msm_weighted_sum, MsmWork::finish) on the CPU emulation build of the HIP sources: zk_msm_stage_probe value
by value against Python integers on the cases of msmstage_cases.py -- the table of window multiples with and without frugal planes, chunks
against bucket boundaries in every lane form, the multi-round branch of ChunkRule::len that only the emulation build's small slot count
reaches, the remap forms of a borrowed sort, buckets of exactly 64 and 65 pieces and the merged tail, and the row / column and weighted
sums at every width that changes their shape on directed bucket contents -- and the probe's refusals.  msmstage_checks.py documents the
checks; test_msmstage_gpu.py runs the same ones on the device.

Measured on the stand-in, 140 tests in 313 s: most cases 0.3 - 3 s; the corner cases at c = 20 4.5 - 5 s (the emulated tail over 2^19
buckets and planes); the cases with n = 2^12 bases at c = 13 (equal_ / alt_) 6 - 7 s on G1, as the slower existing emulation tests, and
13 - 15 s on G2, where the emulated k_msm_precompute inverts 82 k Fq2 elements: those six and the merged tail on G2 (12 s) stand out and
are marked slow.  The refusals take 4 s (some fifty probe calls at c = 3)."""
import ctypes as C
import pytest
import msmstage_cases as cases
import msmstage_checks as chk


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


SLOW = tuple(k for k in cases.CASES if k == "merged_g2_t4" or (k.startswith(("equal_c13_g2", "alt_rows_c13_g2", "alt_cols_c13_g2"))))
assert len(SLOW) == 7


def _params(names):
    return [pytest.param(n, marks=[pytest.mark.slow] if n in SLOW else []) for n in names]


@pytest.mark.parametrize("name", _params(cases.TABLE_CASES))
def test_table_of_window_multiples(zk, oracle, monkeypatch, name):
    chk.check_case(zk, oracle, name, monkeypatch, True)


@pytest.mark.parametrize("name", _params(cases.ACC_CASES))
def test_chunk_pieces(zk, oracle, monkeypatch, name):
    chk.check_case(zk, oracle, name, monkeypatch, True)


@pytest.mark.parametrize("name", _params(cases.HEAVY_CASES))
def test_bucket_sums_and_heavy_list(zk, oracle, monkeypatch, name):
    chk.check_case(zk, oracle, name, monkeypatch, True)


@pytest.mark.parametrize("name", _params(cases.TAIL_CASES))
def test_row_column_and_weighted_sums(zk, oracle, monkeypatch, name):
    chk.check_case(zk, oracle, name, monkeypatch, True)


def test_probe_refusals(zk, oracle, monkeypatch):
    chk.check_refusals(zk, oracle, monkeypatch, True)
