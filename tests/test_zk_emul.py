"""Zero-knowledge proofs (r, s blinding) from the full proving key, on the CPU emulation build of the HIP sources
(libzkhip_emul.so, test infrastructure only): full-key round trip, the closed form of the blinded proof, r = s = 0, the points at
infinity, OS-drawn r, s, and the error cases.  test_zk_gpu.py runs the same checks on the device."""
import filecmp
import numpy as np
import pytest
import pyref
from ethsnarks_amd import r1cs as R, fields as F
from helpers import golden_cases, build_case
import zk_closed_form as Z


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


RS_CASES = [(0x1234567, 0x89abcdef), (1, F.FR - 1), (F.FR - 1, 1)]


def _full_key(zk, r, toxic):
    pk, vk = zk.keygen(r, toxic=toxic, full=True)
    assert pk.is_full()
    return pk, vk


def test_full_key_round_trip(zk, tmp_path):
    case = golden_cases()[0]
    r, w, toxic = build_case(case)
    pk, _ = _full_key(zk, r, toxic)
    f1, f2, nozk = tmp_path / "a.raw", tmp_path / "b.raw", tmp_path / "nozk.raw"
    pk.save_raw_full(str(f1))
    pk2 = zk.load_proving_key(str(f1), full=True)
    assert pk2.is_full()
    pk2.save_raw_full(str(f2))
    assert filecmp.cmp(str(f1), str(f2), shallow=False)
    # the loader is the already-pinned converter plus the G1 half of the B-query
    zk.pk_mcl2nozk(str(f1), str(nozk))
    pk2.save_raw(str(tmp_path / "nozk2.raw"), codec=zk.CODEC_MCL_BN128)
    assert filecmp.cmp(str(nozk), str(tmp_path / "nozk2.raw"), shallow=False)
    for key, val in pk.parts().items():
        got = pk2.parts()[key]
        assert np.array_equal(np.asarray(val), np.asarray(got)), key
    # b1_val[i] = Bt_i G1 with Bt_i the B-query's QAP evaluation at t (pyref.keygen's sums)
    ref_pk, _ = pyref.keygen(r.as_pyref(), *toxic)
    b_idx = pk.parts()["b_idx"].tolist()
    assert b_idx == ref_pk["B"][0]
    nC, nIn, V, _, Brows, _ = r.as_pyref()
    m = pyref.domain_size(nC, nIn)
    t = toxic[0]
    om = pyref.omega(m)
    Zt = (pow(t, m, pyref.R) - 1) % pyref.R
    u = [pow(om, i, pyref.R) * Zt % pyref.R * pow(m * (t - pow(om, i, pyref.R)) % pyref.R, -1, pyref.R) % pyref.R for i in range(m)]
    Bt = [0] * (V + 1)
    for j in range(nC):
        for i, c in Brows[j]:
            Bt[i] = (Bt[i] + u[j] * c) % pyref.R
    b1 = pk.b1_val()
    for row, i in enumerate(b_idx):
        p = pyref.g1_mul(pyref.G1_GEN, Bt[i])
        assert F.fq_from_mont(b1[row].reshape(2, 4)) == [p[0], p[1]], i
    # a nozk key has no full stream
    nz = zk.load_proving_key(str(nozk), codec=zk.CODEC_MCL_BN128)
    assert not nz.is_full()
    with pytest.raises(zk.ZkError) as e:
        nz.save_raw_full(str(tmp_path / "x.raw"))
    assert e.value.code == 1


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_closed_form_golden(zk, case):
    r, w, toxic = build_case(case)
    pk, _ = _full_key(zk, r, toxic)
    ctx = zk.ProverContext(pk, r)
    wm = F.fr_to_mont(w)
    sums = Z.trapdoor_sums(r.as_pyref(), w, *toxic)
    for rr, ss in RS_CASES:
        assert ctx.prove_zk(wm, rs=(rr, ss)) == Z.zk_proof_json(r.as_pyref(), w, toxic, rr, ss, sums)
    assert ctx.prove_zk(F.ints_to_limbs(w), rs=[RS_CASES[0]], canonical=True) == Z.zk_proof_json(r.as_pyref(), w, toxic, *RS_CASES[0], sums)
    # r = s = 0 is the no-ZK proof, byte for byte
    assert ctx.prove_zk(wm, rs=(0, 0)) == zk.prove(ctx, wm) == case["proof_json"]
    ctx.close()


def test_closed_form_chain_2p10(zk):
    r, w = R.synthetic_chain((1 << 10) - 2, 1)
    toxic = [R.SplitMix64(5).fr() for _ in range(5)]
    pk, vk = _full_key(zk, r, toxic)
    ctx = zk.ProverContext(pk, r)
    got = ctx.prove_zk(F.fr_to_mont(w), rs=(12345, 67890))
    assert got == Z.zk_proof_json(r.as_pyref(), w, toxic, 12345, 67890)
    assert zk.stub_verify(vk.to_json(), got)
    ctx.close()


@pytest.mark.parametrize("k", [3, 5])
def test_closed_form_batch(zk, k):
    nC, nIn = 40, 2
    r, _ = R.random_r1cs(nC, nIn, seed=21)
    ws = [R.random_r1cs(nC, nIn, seed=21, witness_seed=100 + i)[1] for i in range(k)]
    toxic = [R.SplitMix64(9).fr() for _ in range(5)]
    pk, vk = _full_key(zk, r, toxic)
    ctx = zk.ProverContext(pk, r, max_batch=k)
    rs = [(1000 + 7 * i, F.FR - 1 - i) for i in range(k)]
    wm = np.stack([F.fr_to_mont(w) for w in ws])
    got = ctx.prove_zk_batch(wm, rs=rs)
    for i in range(k):
        assert got[i] == Z.zk_proof_json(r.as_pyref(), ws[i], toxic, *rs[i]), i
    # the same through submit / collect, r, s as a (k, 8) array
    arr = np.concatenate([F.ints_to_limbs([a, b]).reshape(1, 8) for a, b in rs])
    ctx.submit_zk_batch(wm, rs=arr)
    proofs, _ = ctx.collect_zk_batch(k)
    assert [zk.proof_to_json(p, wm[i, 1:1 + nIn]) for i, p in enumerate(proofs)] == got
    ctx.close()


def test_infinity_edge_cases(zk):
    case = golden_cases()[1]
    r, w, toxic = build_case(case)
    pk, _ = _full_key(zk, r, toxic)
    ctx = zk.ProverContext(pk, r)
    wm = F.fr_to_mont(w)
    sums = Z.trapdoor_sums(r.as_pyref(), w, *toxic)
    rA, sB = Z.r_for_infinite_A(sums, toxic), Z.s_for_infinite_B(sums, toxic)
    for rr, ss in [(rA, 77), (55, sB), (rA, sB), (1, F.FR - 1), (1, 0), (0, F.FR - 1)]:
        got = ctx.prove_zk(wm, rs=(rr, ss))
        assert got == Z.zk_proof_json(r.as_pyref(), w, toxic, rr, ss, sums), (rr, ss)
    both = ctx.prove_zk(wm, rs=(rA, sB))                       # libff's affine image of zero: (0, 1)
    assert ' "A" :["0x0", "0x1"]' in both and ' "B"  :[["0x0", "0x0"],\n ["0x0", "0x1"]]' in both
    ctx.close()


def test_os_randomness(zk):
    case = golden_cases()[2]
    r, w, toxic = build_case(case)
    pk, vk = _full_key(zk, r, toxic)
    ctx = zk.ProverContext(pk, r)
    wm = F.fr_to_mont(w)
    p1, p2 = ctx.prove_zk(wm), ctx.prove_zk(wm)
    a1, _ = zk.proof_from_json(p1)
    a2, _ = zk.proof_from_json(p2)
    assert list(a1.a_x) != list(a2.a_x) and list(a1.b_x_c0) != list(a2.b_x_c0) and list(a1.c_x) != list(a2.c_x)
    vkj = vk.to_json()
    assert zk.stub_verify(vkj, p1) and zk.stub_verify(vkj, p2)
    tampered = p1.replace('"input" :["0x%x"' % w[1], '"input" :["0x%x"' % ((w[1] + 1) % F.FR))
    assert tampered != p1
    assert not zk.stub_verify(vkj, tampered)
    ctx.close()


def test_errors(zk):
    case = golden_cases()[0]
    r, w, toxic = build_case(case)
    wm = F.fr_to_mont(w)
    nozk, _ = zk.keygen(r, toxic=toxic)
    full, _ = _full_key(zk, r, toxic)
    # a nozk-key context
    ctx = zk.ProverContext(nozk, r)
    with pytest.raises(zk.ZkError) as e:
        ctx.prove_zk(wm, rs=(1, 2))
    assert e.value.code == 1 and "full proving key" in str(e.value)
    plain = zk.prove(ctx, wm)
    ctx.close()
    # r >= R, s >= R
    ctx = zk.ProverContext(full, r)
    for bad in [(F.FR, 1), (1, F.FR), ((1 << 256) - 1, 0)]:
        with pytest.raises(zk.ZkError) as e:
            ctx.prove_zk(wm, rs=np.concatenate([F.ints_to_limbs([bad[0]]), F.ints_to_limbs([bad[1]])]).reshape(1, 8))
        assert e.value.code == 1
    # a full key proves without zero knowledge exactly as the nozk key does
    assert zk.prove(ctx, wm) == plain
    # mixing ZK and plain collect
    ctx.submit_zk_batch(wm.reshape(1, -1, 4), rs=[(3, 4)])
    with pytest.raises(zk.ZkError) as e:
        ctx.collect()
    assert e.value.code == 1
    with pytest.raises(zk.ZkError) as e:
        ctx.collect_batch(1)
    assert e.value.code == 1
    proofs, _ = ctx.collect_zk_batch(1)
    assert zk.proof_to_json(proofs[0], wm[1:1 + r.nIn]) == Z.zk_proof_json(r.as_pyref(), w, toxic, 3, 4)
    ctx.submit(wm)
    with pytest.raises(zk.ZkError) as e:
        ctx.collect_zk_batch(1)
    assert e.value.code == 1
    part, _ = ctx.collect()
    assert zk.proof_to_json(ctx.prove_combine(part), wm[1:1 + r.nIn]) == plain
    ctx.close()
    # a sharded context
    ctx = zk.ProverContext(full, r, shard_rank=0, shard_count=2)
    with pytest.raises(zk.ZkError) as e:
        ctx.prove_zk(wm, rs=(1, 2))
    assert e.value.code == 1 and "unsharded" in str(e.value)
    ctx.close()


def test_full_key_context_info_unchanged(zk):
    """a context of the full key chooses what the nozk key's context chooses (zk_ctx_info); its tables add the B1 rows only"""
    case = golden_cases()[3]
    r, w, toxic = build_case(case)
    nozk, _ = zk.keygen(r, toxic=toxic)
    full, _ = _full_key(zk, r, toxic)
    a, b = zk.ProverContext(nozk, r), zk.ProverContext(full, r)
    ia, ib = a.info(), b.info()
    for key in ("A", "B", "H", "L", "share_A", "share_B", "share_L", "m", "planes", "table_rows_B"):
        assert ia[key] == ib[key], key
    assert ib["table_bytes"] == ia["table_bytes"] + 64 * ia["table_rows_B"] * full.nB + (64 + 128) * 43 * 32     # B1, delta1, delta2 (blind.hpp)
    a.close(); b.close()


def test_frugal_tables_closed_form(zk, monkeypatch):
    """a table budget too small for every window: the context keeps every S-th window (S bucket planes) and the blinding kernels fold
    the planes of every MSM result on the device (blind_fold); the proofs of a batch still match the closed form"""
    nC, nIn, k = 40, 2, 3
    r, _ = R.random_r1cs(nC, nIn, seed=31)
    ws = [R.random_r1cs(nC, nIn, seed=31, witness_seed=200 + i)[1] for i in range(k)]
    toxic = [R.SplitMix64(13).fr() for _ in range(5)]
    pk, _ = _full_key(zk, r, toxic)
    monkeypatch.setenv("ZK_TABLE_BUDGET", "1")
    ctx = zk.ProverContext(pk, r, max_batch=k)
    monkeypatch.delenv("ZK_TABLE_BUDGET")
    assert ctx.info()["planes"] > 1
    rs = [(F.FR - 2 - i, 3 + 5 * i) for i in range(k)]
    got = ctx.prove_zk_batch(np.stack([F.fr_to_mont(w) for w in ws]), rs=rs)
    for i in range(k):
        assert got[i] == Z.zk_proof_json(r.as_pyref(), ws[i], toxic, *rs[i]), i
    ctx.close()


def test_cpp_adapter_prove_zk(emul, tmp_path):
    """ethsnarks::load_proving_key_full -> ProverContextT -> ethsnarks::prove_zk -> stub_verify (include/ethsnarks_hip/stubs.hpp),
    compiled with g++ -Werror like test_cpp_frontend.py's program and run against the emulation build"""
    import os, subprocess
    from conftest import ROOT
    exe = str(tmp_path / "zk_frontend_test")
    d = os.path.dirname(emul)
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "zk_frontend_test.cpp"), "-o", exe, "-L" + d, "-lzkhip_emul", "-Wl,-rpath," + d],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([exe, str(tmp_path / "pk.raw"), str(tmp_path / "vk.json")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "VERIFIED", p.stdout + p.stderr
