"""Zero-knowledge proofs (r, s blinding, full proving key) on the MI355X: the closed form of test_zk_emul.py on the device, larger
circuits, the resident witness path, contexts in flight together, and the launch counts."""
import json
import numpy as np
import pytest
import pyref
from ethsnarks_amd import r1cs as R, fields as F
from helpers import golden_cases, build_case
import zk_closed_form as Z

pytestmark = pytest.mark.gpu


def _g1(limbs):
    v = F.fq_from_mont(np.asarray(limbs, dtype=np.uint64).reshape(2, 4))
    return None if v == [0, 0] else (v[0], v[1])


def _g2(limbs):
    v = F.fq_from_mont(np.asarray(limbs, dtype=np.uint64).reshape(4, 4))
    return None if v == [0, 0, 0, 0] else ((v[0], v[1]), (v[2], v[3]))


def _points(proof_json):
    d = json.loads(proof_json)
    inf1 = lambda p: None if p == (0, 1) else p
    b = pyref.g2_from_json(d["B"])
    return inf1(pyref.g1_from_json(d["A"])), (None if b == ((0, 0), (1, 0)) else b), inf1(pyref.g1_from_json(d["C"]))


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_closed_form_golden(hip, case):
    r, w, toxic = build_case(case)
    pk, vk = hip.keygen(r, toxic=toxic, full=True)
    ctx = hip.ProverContext(pk, r)
    wm = F.fr_to_mont(w)
    sums = Z.trapdoor_sums(r.as_pyref(), w, *toxic)
    rA, sB = Z.r_for_infinite_A(sums, toxic), Z.s_for_infinite_B(sums, toxic)
    for rr, ss in [(0x1234567, 0x89abcdef), (1, F.FR - 1), (rA, 5), (7, sB), (rA, sB)]:
        assert ctx.prove_zk(wm, rs=(rr, ss)) == Z.zk_proof_json(r.as_pyref(), w, toxic, rr, ss, sums), (rr, ss)
    assert ctx.prove_zk(wm, rs=(0, 0)) == hip.prove(ctx, wm) == case["proof_json"]
    p1, p2 = ctx.prove_zk(wm), ctx.prove_zk(wm)
    assert p1 != p2
    a1, b1, c1 = _points(p1); a2, b2, c2 = _points(p2)
    assert a1 != a2 and b1 != b2 and c1 != c2
    assert hip.stub_verify(vk.to_json(), p1) and hip.stub_verify(vk.to_json(), p2)
    bad = p1.replace('"input" :["0x%x"' % w[1], '"input" :["0x%x"' % ((w[1] + 1) % F.FR))
    assert bad != p1 and not hip.stub_verify(vk.to_json(), bad)
    ctx.close()


def test_errors_and_launch_counts(hip):
    case = golden_cases()[3]
    r, w, toxic = build_case(case)
    wm = F.fr_to_mont(w)
    nozk, _ = hip.keygen(r, toxic=toxic)
    full, _ = hip.keygen(r, toxic=toxic, full=True)
    cn, cf = hip.ProverContext(nozk, r), hip.ProverContext(full, r)
    with pytest.raises(hip.ZkError) as e:
        cn.prove_zk(wm, rs=(1, 2))
    assert e.value.code == 1
    with pytest.raises(hip.ZkError) as e:
        cf.prove_zk(wm, rs=np.concatenate([F.ints_to_limbs([F.FR]), F.ints_to_limbs([1])]).reshape(1, 8))
    assert e.value.code == 1
    hip.prove(cn, wm); hip.prove(cf, wm); cf.prove_zk(wm, rs=(1, 2))           # (warm: lazily created events, H stream)
    n0 = hip.launch_count(); a = hip.prove(cn, wm); n1 = hip.launch_count(); b = hip.prove(cf, wm); n2 = hip.launch_count()
    z = cf.prove_zk(wm, rs=(3, 4)); n3 = hip.launch_count()
    assert a == b and n2 - n1 == n1 - n0, (n1 - n0, n2 - n1)
    extra = (n3 - n2) - (n1 - n0)
    print("launches per proof: nozk %d, zero-knowledge %d (+%d: B1 accumulation and tail, k_zk_blind_fixed / _g1 / _g2)" % (n1 - n0, n3 - n2, extra))
    assert extra == 8              # one G1 accumulation, its four-kernel tail (finalize, heavy, row / column, weighted), three blinding kernels
    assert z == Z.zk_proof_json(r.as_pyref(), w, toxic, 3, 4)
    cf.submit_zk_batch(wm.reshape(1, -1, 4), rs=[(5, 6)])
    with pytest.raises(hip.ZkError):
        cf.collect()
    proofs, _ = cf.collect_zk_batch(1)
    assert hip.proof_to_json(proofs[0], wm[1:1 + r.nIn]) == Z.zk_proof_json(r.as_pyref(), w, toxic, 5, 6)
    cs = hip.ProverContext(full, r, shard_rank=0, shard_count=2)
    with pytest.raises(hip.ZkError) as e:
        cs.prove_zk(wm, rs=(1, 2))
    assert e.value.code == 1
    cs.close(); cn.close(); cf.close()


def test_chain_2p16_closed_form(hip):
    r, w = R.synthetic_chain((1 << 16) - 2, 1)
    toxic = [R.SplitMix64(16).fr() for _ in range(5)]
    pk, vk = hip.keygen(r, toxic=toxic, full=True)
    ctx = hip.ProverContext(pk, r)
    got = ctx.prove_zk(F.fr_to_mont(w), rs=(0xdeadbeef, 0xfeedface))
    assert got == Z.zk_proof_json(r.as_pyref(), w, toxic, 0xdeadbeef, 0xfeedface)
    assert hip.stub_verify(vk.to_json(), got)
    ctx.close()


def test_merkle29_batch_and_resident(hip):
    from ethsnarks_amd import gadgets as G
    k = 32
    cases = [G.merkle_membership_circuit(29)] + [
        G.merkle_membership_circuit(29, leaf=3000 + p, address=(0x15555555 * (p + 1)) & ((1 << 29) - 1), path=[G.merkle_unique(d, 5 + p) for d in range(29)])
        for p in range(1, k)]
    r = cases[0][0]
    toxic = [R.SplitMix64(29).fr() for _ in range(5)]
    pk, vk = hip.keygen(r, toxic=toxic, full=True)
    ctx = hip.ProverContext(pk, r, max_batch=k)
    wm = np.stack([F.fr_to_mont(c[1]) for c in cases])
    rs = [((p + 1) * 0x1000193, F.FR - 3 - p) for p in range(k)]
    got = ctx.prove_zk_batch(wm, rs=rs)
    rp = r.as_pyref()
    for p in (0, 1, 17, k - 1):
        assert got[p] == Z.zk_proof_json(rp, cases[p][1], toxic, *rs[p]), p
    vkj = vk.to_json()
    assert all(hip.stub_verify(vkj, g) for g in got)
    # zk_wplan_solve -> zk_prove_zk_batch_submit_resident: the witnesses never visit the host
    kr = 4
    supplied = list(range(0, 1 + 1 + 29 + 29 + 1 + 29))
    plan = hip.WitnessPlan(r, supplied)
    start = np.zeros((kr, r.V + 1, 4), dtype=np.uint64)
    for p in range(kr):
        start[p, supplied] = wm[p][supplied]
    buf = hip.DeviceBuffer(32 * (r.V + 1) * kr)
    buf.upload(start)
    assert plan.solve(buf.ptr, kr) == 0
    ctx.submit_zk_batch(device_ptr=buf.ptr, k=kr, rs=rs[:kr])
    proofs, _ = ctx.collect_zk_batch(kr)
    assert [hip.proof_to_json(pr, wm[p, 1:1 + r.nIn]) for p, pr in enumerate(proofs)] == got[:kr]
    ctx.close(); plan.close(); buf.free()


def test_two_contexts_in_flight(hip):
    case = golden_cases()[2]
    r, w, toxic = build_case(case)
    pk, _ = hip.keygen(r, toxic=toxic, full=True)
    c1, c2 = hip.ProverContext(pk, r), hip.ProverContext(pk, r)
    wm = F.fr_to_mont(w).reshape(1, -1, 4)
    c1.submit_zk_batch(wm, rs=[(11, 12)]); c2.submit_zk_batch(wm, rs=[(13, 14)])
    (p2,), _ = c2.collect_zk_batch(1); (p1,), _ = c1.collect_zk_batch(1)
    for (rr, ss), pr in (((11, 12), p1), ((13, 14), p2)):
        assert hip.proof_to_json(pr, wm[0, 1:1 + r.nIn]) == Z.zk_proof_json(r.as_pyref(), w, toxic, rr, ss)
    c1.close(); c2.close()


@pytest.mark.parametrize("logm", [18, 20])
def test_large_chain_against_the_nozk_proof(hip, oracle, logm):
    """the ZK proof against the no-ZK proof in closed form from the toxic waste (the C oracle's proof_from_trapdoor):
    A0 + r delta1, B0 + s delta2, C0 + s A0 + r B1_0 + r s delta1 with B1_0 = beta1 + sum w_i B1_i (the C oracle's multi-exponentiation)"""
    r, w = R.synthetic_chain((1 << logm) - 2, 1)
    rng = R.SplitMix64(logm)
    toxic = [rng.fr() for _ in range(5)]
    pk, vk = hip.keygen(r, toxic=toxic, full=True)
    ctx = hip.ProverContext(pk, r)
    wm = F.fr_to_mont(w)
    rr, ss = 0x0123456789abcdef0123456789abcdef, F.FR - 0x5555
    z0, z = ctx.prove_zk(wm, rs=(0, 0)), ctx.prove_zk(wm, rs=(rr, ss))
    assert z0 == oracle.proof_from_trapdoor(r, wm, toxic)
    parts = pk.parts()
    d1, d2, b1 = _g1(parts["delta_g1"]), _g2(parts["delta_g2"]), _g1(parts["beta_g1"])
    A0, B0, C0 = _points(z0)
    A, B, Cz = _points(z)
    assert A == pyref.g1_add(A0, pyref.g1_mul(d1, rr))
    assert B == pyref.g2_add(B0, pyref.g2_mul(d2, ss))
    B1_0 = pyref.g1_add(b1, _g1(oracle.msm(pk.b1_val(), wm[parts["b_idx"].astype(np.int64)])))
    want = pyref.g1_add(C0, pyref.g1_add(pyref.g1_mul(A0, ss), pyref.g1_add(pyref.g1_mul(B1_0, rr), pyref.g1_mul(d1, rr * ss % F.FR))))
    assert Cz == want
    assert hip.stub_verify(vk.to_json(), z)
    ctx.close()


def test_cpp_adapter_prove_zk(tmp_path):
    """ethsnarks::load_proving_key_full -> ProverContextT -> ethsnarks::prove_zk -> stub_verify, linked against libzkhip.so"""
    import os, subprocess
    from conftest import ROOT
    exe = str(tmp_path / "zk_frontend_test")
    lib = os.path.join(ROOT, "ethsnarks_amd")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "zk_frontend_test.cpp"), "-o", exe, "-L" + lib, "-lzkhip", "-Wl,-rpath," + lib],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([exe, str(tmp_path / "pk.raw"), str(tmp_path / "vk.json")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "VERIFIED", p.stdout + p.stderr
