"""Batch Groth16 verification on the device (zk_vctx / zk_verify_batch*, zk_pairing_check): the verdict tests of
test_verify_batch_emul.py against libzkhip.so on an MI355X, batches that fill more than one wave per CU, proofs straight from
zk_prove_batch / zk_prove_zk_batch, and the C++ adapter.  Every GPU step runs once."""
import json
import os
import subprocess
import numpy as np
import pytest
import pyref
from ethsnarks_amd import r1cs as R, fields as F
from helpers import golden_cases, build_case, GOLDEN
import verify_batch_cases as V

pytestmark = pytest.mark.gpu


def _second_proof(hip, case, r, toxic):
    if case["kind"] == "chain":
        _, w2 = R.synthetic_chain(case["nC"], case["nIn"], case["seed"] + 1)
    else:
        _, w2 = R.random_r1cs(case["nC"], case["nIn"], seed=case["seed"], small_values=case["small_values"], witness_seed=977)
    pk, _ = hip.keygen(r, toxic=toxic)
    ctx = hip.ProverContext(pk, r)
    p2 = hip.prove(ctx, F.fr_to_mont(w2))
    ctx.close()
    return p2


def test_pairing_check_bilinearity(hip):
    rng = R.SplitMix64(53)
    G1, G2 = pyref.G1_GEN, pyref.G2_GEN
    groups, want = [], []
    for i in range(70):                                                                 # more than one wave
        a, b = rng.fr(), rng.fr()
        good = i % 3 != 1
        c = a * b % pyref.R if good else (a * b + 1) % pyref.R
        P = pyref.g1_mul(G1, a) if i != 5 else None                                     # infinity as an operand: e(O, bQ) e(-cP, Q)
        if i == 5:
            c, good = 0, True
        groups.append([(P, pyref.g2_mul(G2, b)), (pyref.g1_neg(pyref.g1_mul(G1, c)) if c else None, G2)])
        want.append(good)
    g1 = np.stack([V.g1_limbs(p) for g in groups for p, _ in g])
    g2 = np.stack([V.g2_limbs(q) for g in groups for _, q in g])
    assert hip.pairing_check(g1, g2, 2) == want
    assert pyref.pairing_product_is_one(groups[0]) and not pyref.pairing_product_is_one(groups[1])
    # n = 1, 3, 4 against pyref
    for n in (1, 3, 4):
        sc = [(rng.fr(), rng.fr()) for _ in range(n)]
        pairs = [(pyref.g1_mul(G1, a), pyref.g2_mul(G2, b)) for a, b in sc]
        one = list(pairs)
        one[-1] = (pyref.g1_neg(pyref.g1_mul(G1, sum(a * b for a, b in sc[:-1]) % pyref.R)), G2) if n > 1 else (None, G2)
        gs = [pairs, one]
        g1 = np.stack([V.g1_limbs(p) for g in gs for p, _ in g])
        g2 = np.stack([V.g2_limbs(q) for g in gs for _, q in g])
        assert hip.pairing_check(g1, g2, n) == [pyref.pairing_product_is_one(g) for g in gs] == [False, True], n


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_verify_batch_golden(hip, case):
    r, w, toxic = build_case(case)
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    p2 = _second_proof(hip, case, r, toxic)
    s1, s2 = V.swap_inputs(valid, p2)
    bad = [V.tamper_pairing(k, valid) for k in V.PAIRING_KINDS] + [s1, s2]
    forms = [t for t in (V.tamper_form(k, valid, seed=5 + i) for i, k in enumerate(V.FORM_KINDS)) if t is not None]
    texts = V.interleave(valid, bad + forms) + [p2]
    want = V.expected(hip, vkj, texts)
    assert want == [True, False] * (len(bad) + len(forms)) + [True]
    assert pyref.verify(case["vk"], V.as_dict(valid)) and not pyref.verify(case["vk"], V.as_dict(bad[0]))
    verifier = hip.Verifier(vkj, max_batch=len(texts))
    assert verifier.verify(texts) == want
    rot = texts[1:] + texts[:1]
    assert verifier.verify(rot) == want[1:] + want[:1]
    verifier.close()


def test_subgroup_and_infinity(hip):
    case = golden_cases()[1]
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    A, B, Cc, inp = V.parse(valid)
    cof = 2 * pyref.Q - pyref.R
    base = V.twist_point_outside_subgroup(11)
    low = V.g2_mul_raw(base, cof * pyref.R // 10069)
    assert low is not None and V.g2_mul_raw(low, 10069) is None
    pts = [base, low, pyref.g2_add(B, low)]
    z1, z2 = (0, 0), ((0, 0), (0, 0))
    texts = []
    for pt in pts:
        texts += [V.text(A, pt, Cc, inp), valid]
    texts += [V.text(z1, B, Cc, inp), V.text(A, z2, Cc, inp), V.text(A, B, z1, inp), V.text(None, B, Cc, inp)]
    want = V.expected(hip, vkj, texts)
    assert want == [False, True] * 3 + [False] * 4
    verifier = hip.Verifier(vkj, max_batch=len(texts))
    assert verifier.verify(texts) == want
    recs, inps = zip(*[hip.proof_from_json(t) for t in texts[:9]])
    assert verifier.verify_structs(list(recs), np.stack(inps)) == want[:9]
    verifier.close()


def test_mimc_batch_of_64_one_corrupted(hip):
    """64 MiMC-preimage proofs from zk_prove_batch verified in one call, one of them corrupted in the middle"""
    from ethsnarks_amd import gadgets as G
    k = 64
    r1cs, w0, _ = G.mimc_preimage_circuit(11)
    ws = [w0] + [G.mimc_preimage_circuit(11, seed=7 + p)[1] for p in range(1, k)]
    pk, vk = hip.keygen(r1cs, seed=R.SEED_DEFAULT)
    ctx = hip.ProverContext(pk, r1cs, max_batch=k)
    proofs = hip.prove_batch(ctx, np.stack([F.fr_to_mont(w) for w in ws]))
    ctx.close()
    verifier = hip.Verifier(vk, max_batch=k)
    assert verifier.verify(proofs) == [True] * k
    bad = list(proofs)
    bad[37] = V.tamper_pairing("C+G", proofs[37])
    assert verifier.verify(bad) == [i != 37 for i in range(k)]
    vkj = vk.to_json()
    assert hip.stub_verify(vkj, proofs[37]) and not hip.stub_verify(vkj, bad[37])
    verifier.close()


def test_batch_larger_than_one_wave_per_cu(hip):
    """k = 4 096 + 1 variants of a few proofs, tampered at seeded positions: the grid mapping, a ragged last wave, k = max_batch"""
    case = golden_cases()[3]
    r, w, toxic = build_case(case)
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    p2 = _second_proof(hip, case, r, toxic)
    pool = [(valid, True), (p2, True), (V.tamper_pairing("A2", valid), False), (V.tamper_pairing("input", p2), False),
            (V.tamper_form("B outside subgroup", valid, seed=3), False), (V.tamper_form("coord>=q", p2), False)]
    assert V.expected(hip, vkj, [t for t, _ in pool]) == [ok for _, ok in pool]
    k = 4097
    rng = R.SplitMix64(97)
    pick = [rng.next() % len(pool) for _ in range(k)]
    pick[0], pick[63], pick[64], pick[4095], pick[4096] = 2, 0, 3, 1, 2
    verifier = hip.Verifier(vkj, max_batch=k)
    got = verifier.verify([pool[i][0] for i in pick])
    want = [pool[i][1] for i in pick]
    assert got == want
    assert 0 < sum(want) < k
    with pytest.raises(hip.ZkError) as e:
        verifier.verify([valid] * (k + 1))
    assert e.value.code == 1
    assert verifier.verify([valid]) == [True]                                           # k = 1 on the same context
    verifier.close()


def test_zero_knowledge_batch(hip):
    case = golden_cases()[2]
    r, w, toxic = build_case(case)
    pk, vk = hip.keygen(r, toxic=toxic, full=True)
    ctx = hip.ProverContext(pk, r, max_batch=4)
    wm = F.fr_to_mont(w)
    proofs = ctx.prove_zk_batch(np.stack([wm] * 4))                                     # r, s from the operating system
    ctx.close()
    assert len(set(proofs)) == 4
    texts = proofs[:2] + [V.tamper_pairing("B+G2", proofs[2])] + proofs[3:]
    assert hip.stub_verify_batch(vk.to_json(), texts) == V.expected(hip, vk.to_json(), texts) == [True, True, False, True]


@pytest.mark.parametrize("nIn", [0, 3])
def test_input_counts_and_fallback(hip, nIn, monkeypatch):
    nC = 12
    r, w = R.random_r1cs(nC, nIn, seed=60 + nIn)
    _, w2 = R.random_r1cs(nC, nIn, seed=60 + nIn, witness_seed=71)
    pk, vk = hip.keygen(r, toxic=[R.SplitMix64(17 + nIn).fr() for _ in range(5)])
    ctx = hip.ProverContext(pk, r)
    p1, p2 = hip.prove(ctx, F.fr_to_mont(w)), hip.prove(ctx, F.fr_to_mont(w2))
    ctx.close()
    vkj = vk.to_json()
    texts = [p1, V.tamper_pairing("input", p1), p2, V.tamper_pairing("C+G", p2)] + (list(V.swap_inputs(p1, p2)) if nIn else [])
    want = V.expected(hip, vkj, texts)
    assert want[:4] == [True, False, True, False] and not any(want[4:])
    verifier = hip.Verifier(vk, max_batch=len(texts))
    assert verifier.verify(texts) == want
    verifier.close()
    monkeypatch.setenv("ZK_VERIFY_TABLE_BUDGET", "1")
    verifier = hip.Verifier(vk, max_batch=len(texts))
    monkeypatch.delenv("ZK_VERIFY_TABLE_BUDGET")
    assert verifier.verify(texts) == want
    verifier.close()


def test_reference_static_triple(hip):
    d = json.load(open(os.path.join(GOLDEN, "ref_static_triple.json")))
    vkj = json.dumps(d["vk"])
    valid = json.dumps(d["proof"])
    texts = [json.dumps(dict(d["proof"], input=[d["proof"]["input"][0], "0x8"])), valid, json.dumps(dict(d["proof"], A=d["proof"]["C"])), valid]
    assert hip.stub_verify_batch(vkj, texts) == V.expected(hip, vkj, texts) == [False, True, False, True]


def test_cpp_adapter_verify_batch(hip, tmp_path):
    """ethsnarks::stub_verify_batch (include/ethsnarks_hip/stubs.hpp) linked against libzkhip.so"""
    from conftest import ROOT
    exe = str(tmp_path / "verify_batch_test")
    lib = os.path.join(ROOT, "ethsnarks_amd")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "verify_batch_test.cpp"), "-o", exe, "-L" + lib, "-lzkhip", "-Wl,-rpath," + lib],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    case = golden_cases()[0]
    vkf, pf, bf = tmp_path / "vk.json", tmp_path / "proof.json", tmp_path / "bad.json"
    vkf.write_text(json.dumps(case["vk"])); pf.write_text(case["proof_json"]); bf.write_text(V.tamper_pairing("A2", case["proof_json"]))
    p = subprocess.run([exe, str(vkf), str(pf), str(bf)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "BATCH OK", p.stdout + p.stderr
