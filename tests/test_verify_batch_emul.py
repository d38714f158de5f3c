"""Batch Groth16 verification (zk_vctx / zk_verify_batch*, zk_pairing_check; csrc/pairing.hpp, verify_gpu.cpp) on the CPU emulation build of
the HIP sources: the tower and the pairing against oracle/pyref.py, the verdicts against the host verifier zk_verify and pyref.verify.
test_verify_batch_gpu.py runs the verdict tests on the device."""
import ctypes as C
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import pyref
from ethsnarks_amd import r1cs as R, fields as F
from helpers import golden_cases, build_case, GOLDEN
import verify_batch_cases as V


@pytest.fixture(scope="module")
def emul_verify(emul):
    """the verifier unit of the CPU emulation build (tests/emul_verify): a library of its own beside libzkhip_emul.so, which it depends on"""
    from conftest import ROOT
    d = os.path.join(ROOT, "tests", "emul_verify")
    so = os.path.join(d, "libzkhip_emul_verify.so")
    csrc = os.path.join(ROOT, "ethsnarks_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith("pp")] + [emul, os.path.join(d, "Makefile")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", d, "-s"])
    return so


@pytest.fixture(scope="module")
def zk(emul_verify):
    from ethsnarks_amd import prover
    prover._lib = None
    prover._lib_path_loaded = None
    prover.load_library(emul_verify)
    assert b"EMULATION" in prover._lib.zk_version()
    yield prover
    prover._lib = None
    prover._lib_path_loaded = None


# ---------------------------------------------------------------- the tower
def test_tower_against_pyref(zk):
    rng = R.SplitMix64(41)
    for _ in range(3):
        a, b = V.tower_random(rng), V.tower_random(rng)
        pa, pb = V.tower_to_pyref(a), V.tower_to_pyref(b)
        assert V.tower_to_pyref(V.tower_call(zk, 0, a, b)) == pyref.f12_mul(pa, pb)
        assert V.tower_to_pyref(V.tower_call(zk, 1, a)) == pyref.f12_mul(pa, pa)
        assert pyref.f12_mul(V.tower_to_pyref(V.tower_call(zk, 2, a)), pa) == pyref.F12_ONE
        for k in (1, 2, 3):
            assert V.tower_to_pyref(V.tower_call(zk, 2 + k, a)) == pyref.f12_pow(pa, pyref.Q ** k), k
        assert V.tower_to_pyref(V.tower_call(zk, 9, a)) == pyref.f12_pow(pa, pyref.Q ** 6)
    # sparse operands and the units
    one = [1] + [0] * 11
    assert V.tower_call(zk, 0, one, a) == a and V.tower_call(zk, 2, one) == one
    assert V.tower_call(zk, 2, [0] * 12) == [0] * 12                                   # 1/0 is 0: no fault, no trap


def test_frobenius_constants(zk):
    """the coefficient the q^k map puts on v^i w^j is xi^((2i + j)(q^k - 1)/6)"""
    for k in (1, 2, 3):
        for j in range(2):
            for i in range(3):
                e = [0] * 12
                e[2 * (3 * j + i)] = 1
                got = V.tower_call(zk, 2 + k, e)
                want = pyref.f2_pow(pyref.XI, (pyref.Q ** k - 1) // 6 * (2 * i + j))
                assert (got[2 * (3 * j + i)], got[2 * (3 * j + i) + 1]) == want, (k, i, j)
                assert sum(1 for v in got if v) == sum(1 for v in want if v)


def test_constants_header_is_generated():
    from conftest import ROOT
    d = os.path.join(ROOT, "ethsnarks_amd", "csrc")
    out = subprocess.run([sys.executable, os.path.join(d, "gen_pairing_consts.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(d, "pairing_consts.hpp")).read()
    # and its values are pyref's: the twist's b and 1/2 (the Frobenius coefficients: test_frobenius_constants)
    mont = lambda v: ", ".join("0x%08xu" % ((v * (1 << 256) % pyref.Q >> (32 * i)) & 0xffffffff) for i in range(8))
    assert "twist_b() { fe2 r = {{{%s}}, {{%s}}}" % (mont(pyref.TWIST_B[0]), mont(pyref.TWIST_B[1])) in out
    assert "two_inv() { fe r = {{%s}}" % mont(pow(2, -1, pyref.Q)) in out


def test_cyclotomic_square_and_final_exponentiation(zk):
    rng = R.SplitMix64(43)
    a = V.tower_random(rng)
    pa = V.tower_to_pyref(a)
    g = V.tower_call(zk, 7, a)                                                          # into the cyclotomic subgroup
    assert V.tower_to_pyref(g) == pyref.f12_pow(pa, (pyref.Q ** 6 - 1) * (pyref.Q ** 2 + 1))
    assert V.tower_call(zk, 6, g) == V.tower_call(zk, 1, g)
    assert V.tower_call(zk, 6, a) != V.tower_call(zk, 1, a)                             # (outside it the two differ)
    # the chain computes a fixed power of the true value, coprime to r
    import math
    assert math.gcd(V.FE_CHAIN_POWER, pyref.R) == 1
    assert V.tower_to_pyref(V.tower_call(zk, 8, a)) == pyref.f12_pow(pyref.final_exp(pa), V.FE_CHAIN_POWER)


# ---------------------------------------------------------------- zk_pairing_check
def _check(zk, groups):
    """groups: list of lists of (P, Q) pairs, all of one length n; returns the library's verdicts"""
    n = len(groups[0])
    g1 = np.stack([V.g1_limbs(p) for g in groups for p, _ in g])
    g2 = np.stack([V.g2_limbs(q) for g in groups for _, q in g])
    return zk.pairing_check(g1, g2, n)


def test_pairing_check_against_pyref(zk):
    rng = R.SplitMix64(47)
    G1, G2 = pyref.G1_GEN, pyref.G2_GEN
    for n in (1, 2, 3, 4):
        groups = []
        for trial in range(3):
            sc = [(rng.fr(), rng.fr()) for _ in range(n)]
            pairs = [(pyref.g1_mul(G1, a), pyref.g2_mul(G2, b)) for a, b in sc]
            if trial == 0 and n > 1:                                                    # make the product one: last pair cancels the others
                tot = sum(a * b for a, b in sc[:-1]) % pyref.R
                pairs[-1] = (pyref.g1_neg(pyref.g1_mul(G1, tot)), G2)
            if trial == 1:                                                              # infinity as an operand
                pairs[0] = (None, pairs[0][1]) if n % 2 else (pairs[0][0], None)
            groups.append(pairs)
        if n == 1:
            groups.append([(None, G2)]); groups.append([(G1, None)]); groups.append([(None, None)])
        want = [pyref.pairing_product_is_one(g) for g in groups]
        assert _check(zk, groups) == want, n
        if n > 1:
            assert want[0] is True and want[2] is False
        else:
            assert want == [False, True, False, True, True, True]


def test_pairing_bilinearity_sweep(zk):
    """e(aP, bQ) e(-abP, Q) = 1 needs no oracle: 24 seeded (a, b), the odd positions perturbed so that every lane position of the launch
    sees both answers"""
    rng = R.SplitMix64(53)
    G1, G2 = pyref.G1_GEN, pyref.G2_GEN
    for flip in (0, 1):
        groups, want = [], []
        for i in range(24):
            a, b = rng.fr(), rng.fr()
            if i < 4:
                a, b = [(1, 1), (pyref.R - 1, 2), (2, pyref.R - 1), (0, 5)][i]
            good = (i + flip) % 2 == 0
            c = a * b % pyref.R if good else (a * b + 1) % pyref.R
            groups.append([(pyref.g1_mul(G1, a), pyref.g2_mul(G2, b)), (pyref.g1_neg(pyref.g1_mul(G1, c)), G2)])
            want.append(good)
        assert _check(zk, groups) == want


def test_pairing_check_errors(zk):
    g1 = np.zeros((1, 8), dtype=np.uint64); g2 = np.zeros((1, 16), dtype=np.uint64)
    out = (C.c_uint8 * 1)()
    L = zk._lib
    assert L.zk_pairing_check(None, zk._p64(g2), C.c_uint32(1), C.c_uint32(1), 0, out) == 1
    assert L.zk_pairing_check(zk._p64(g1), zk._p64(g2), C.c_uint32(0), C.c_uint32(1), 0, out) == 1
    assert L.zk_pairing_check(zk._p64(g1), zk._p64(g2), C.c_uint32(1), C.c_uint32(0), 0, out) == 1
    assert L.zk_pairing_check(zk._p64(g1), zk._p64(g2), C.c_uint32(1), C.c_uint32(1), 0, None) == 1


# ---------------------------------------------------------------- zk_verify_batch
def _second_proof(zk, case, r, toxic):
    """a proof of another witness of the case's circuit, under the same key"""
    if case["kind"] == "chain":
        _, w2 = R.synthetic_chain(case["nC"], case["nIn"], case["seed"] + 1)
    else:
        _, w2 = R.random_r1cs(case["nC"], case["nIn"], seed=case["seed"], small_values=case["small_values"], witness_seed=977)
    pk, _ = zk.keygen(r, toxic=toxic)
    ctx = zk.ProverContext(pk, r)
    p2 = zk.prove(ctx, F.fr_to_mont(w2))
    ctx.close()
    return p2


def _both_rotations(zk, verifier, vkj, texts):
    """the batch and its rotation by one against the host verifier; returns the host verdicts of `texts`"""
    want = V.expected(zk, vkj, texts)
    assert verifier.verify(texts) == want
    rot = texts[1:] + texts[:1]
    assert verifier.verify(rot) == want[1:] + want[:1]
    return want


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_verify_batch_golden(zk, case):
    r, w, toxic = build_case(case)
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    p2 = _second_proof(zk, case, r, toxic)
    s1, s2 = V.swap_inputs(valid, p2)
    bad = [V.tamper_pairing(k, valid) for k in V.PAIRING_KINDS] + [s1, s2]
    texts = V.interleave(valid, bad) + [p2]
    verifier = zk.Verifier(vkj, max_batch=len(texts))
    want = _both_rotations(zk, verifier, vkj, texts)
    assert want == [True, False] * len(bad) + [True]
    # the independent oracle: the valid proofs and one tampered proof of every kind
    assert pyref.verify(case["vk"], V.as_dict(valid)) and pyref.verify(case["vk"], V.as_dict(p2))
    for t in bad:
        assert not pyref.verify(case["vk"], V.as_dict(t))
    # these stay in their groups: only the pairing equation rejects them
    for t in bad:
        A, B, Cc, _ = V.parse(t)
        assert pyref.g1_on_curve(A) and pyref.g1_on_curve(Cc) and pyref.g2_on_curve(B) and V.g2_mul_raw(B, pyref.R) is None
    verifier.close()


@pytest.mark.parametrize("case", golden_cases()[:2], ids=lambda c: c["name"])
def test_verify_batch_ill_formed(zk, case):
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    bad = [t for t in (V.tamper_form(k, valid, seed=5 + i) for i, k in enumerate(V.FORM_KINDS)) if t is not None]
    assert len(bad) == len(V.FORM_KINDS)
    texts = V.interleave(valid, bad)
    verifier = zk.Verifier(vkj, max_batch=len(texts))
    want = _both_rotations(zk, verifier, vkj, texts)
    assert want == [True, False] * len(bad)
    outside = V.parse(bad[V.FORM_KINDS.index("B outside subgroup")])[1]
    assert pyref.g2_on_curve(outside) and V.g2_mul_raw(outside, pyref.R) is not None
    assert not pyref.verify(case["vk"], V.as_dict(bad[V.FORM_KINDS.index("B outside subgroup")]))
    assert not pyref.verify(case["vk"], V.as_dict(bad[V.FORM_KINDS.index("A off curve")]))
    verifier.close()


def test_subgroup_check_pinned_to_r_times_B(zk):
    """several twist points outside the order-r subgroup, among them low-order ones (cofactor multiples) where an incomplete addition
    chain would meet T = O or T = +-B early: verdict 0 for each, as [r]B != O demands, and the neighbours keep theirs"""
    case = golden_cases()[1]
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    A, B, Cc, inp = V.parse(valid)
    cof = 2 * pyref.Q - pyref.R
    small = [p for p in (10069, 5864401) if cof % p == 0]
    assert small, "the known small factors of the twist's cofactor"
    pts = [V.twist_point_outside_subgroup(s) for s in (11, 12, 13)]
    base = pts[0]
    n_all = cof * pyref.R
    for p in small:                                                                     # a point of order p
        lp = V.g2_mul_raw(base, n_all // p)
        assert lp is not None and V.g2_mul_raw(lp, p) is None
        pts.append(lp)
        pts.append(pyref.g2_add(B, lp))                                                 # order p r
    texts = []
    for pt in pts:
        assert pyref.g2_on_curve(pt) and V.g2_mul_raw(pt, pyref.R) is not None
        texts += [V.text(A, pt, Cc, inp), valid]
    verifier = zk.Verifier(vkj, max_batch=len(texts))
    assert verifier.verify(texts) == V.expected(zk, vkj, texts) == [False, True] * len(pts)
    verifier.close()


def test_infinity_operands_and_struct_route(zk):
    """(0, 0) is the point at infinity for zk_verify (factor 1, not an error); the (0, 1) the prover writes for an infinite point is rejected"""
    case = golden_cases()[0]
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    A, B, Cc, inp = V.parse(valid)
    z1, z2 = (0, 0), ((0, 0), (0, 0))
    texts = [V.text(z1, B, Cc, inp), valid, V.text(A, z2, Cc, inp), V.text(A, B, z1, inp), V.text(z1, z2, z1, inp), V.text(None, B, Cc, inp), V.text(A, None, Cc, inp)]
    verifier = zk.Verifier(vkj, max_batch=16)
    want = V.expected(zk, vkj, texts)
    assert verifier.verify(texts) == want and want[1] is True and not any(want[:1] + want[2:])
    # struct route: the same records, then the flags
    recs, inps = [], []
    for t in texts[:5]:
        p, i = zk.proof_from_json(t)
        recs.append(p); inps.append(i)
    assert verifier.verify_structs(recs, np.stack(inps)) == want[:5]
    # what the prover writes for an infinite point: (0, 1) beside the flag -- on neither curve, rejected like its text; the flag alone
    # changes nothing (zk_proof_to_json prints the coordinates)
    for flag, coords in (("a_inf", ("a_x", "a_y")), ("b_inf", ("b_x_c0", "b_x_c1", "b_y_c0", "b_y_c1")), ("c_inf", ("c_x", "c_y"))):
        p, i = zk.proof_from_json(valid)
        q, _ = zk.proof_from_json(valid)
        f, _ = zk.proof_from_json(valid)
        setattr(p, flag, 1); setattr(f, flag, 1)
        for name in coords:
            for j in range(4):
                getattr(p, name)[j] = 1 if (j == 0 and name in ("a_y", "b_y_c0", "c_y")) else 0
        host = [zk.stub_verify(vkj, zk.proof_to_json(x, i, canonical=True)) for x in (q, p, f, q)]
        assert host == [True, False, True, True]
        assert verifier.verify_structs([q, p, f, q], np.stack([i, i, i, i])) == host
    # struct route: a coordinate >= q, an input >= r
    p, i = zk.proof_from_json(valid)
    q, _ = zk.proof_from_json(valid)
    big = F.ints_to_limbs([A[1] + pyref.Q])[0]
    for j in range(4):
        p.a_y[j] = int(big[j])
    i2 = i.copy(); i2[0] = F.ints_to_limbs([inp[0] + pyref.R])[0]
    assert verifier.verify_structs([p, q, q], np.stack([i, i, i2])) == [False, True, False]
    verifier.close()


def test_verify_batch_zero_knowledge_proofs(zk):
    case = golden_cases()[2]
    r, w, toxic = build_case(case)
    pk, vk = zk.keygen(r, toxic=toxic, full=True)
    ctx = zk.ProverContext(pk, r, max_batch=3)
    wm = F.fr_to_mont(w)
    proofs = ctx.prove_zk_batch(np.stack([wm, wm, wm]))                                 # r, s from the operating system
    assert len(set(proofs)) == 3
    tampered = V.tamper_pairing("input", proofs[1])
    verifier = zk.Verifier(vk, max_batch=4)                                             # a VerificationKey object
    texts = [proofs[0], tampered, proofs[1], proofs[2]]
    assert verifier.verify(texts) == V.expected(zk, vk.to_json(), texts) == [True, False, True, True]
    assert zk.stub_verify_batch(vk.to_json(), texts) == [True, False, True, True]
    verifier.close(); ctx.close()


def test_batch_sizes_and_errors(zk):
    case = golden_cases()[0]
    vkj = json.dumps(case["vk"])
    valid = case["proof_json"]
    bad = V.tamper_pairing("A2", valid)
    verifier = zk.Verifier(vkj, max_batch=5)
    assert verifier.verify([valid]) == [True] and verifier.verify([bad]) == [False]     # k = 1
    full = [valid, bad, bad, valid, bad]                                                # k = max_batch
    assert verifier.verify(full) == [True, False, False, True, False]
    with pytest.raises(zk.ZkError) as e:                                                # k > max_batch
        verifier.verify(full + [valid])
    assert e.value.code == 1
    with pytest.raises(zk.ZkError) as e:                                                # k = 0
        verifier.verify([])
    assert e.value.code == 1
    L = zk._lib
    p, i = zk.proof_from_json(valid)
    out = (C.c_uint8 * 1)()
    arr = (C.c_char_p * 1)(valid.encode())
    assert L.zk_verify_batch(None, C.byref(p), zk._p64(i), C.c_uint32(1), out) == 1
    assert L.zk_verify_batch(verifier._h, None, zk._p64(i), C.c_uint32(1), out) == 1
    assert L.zk_verify_batch(verifier._h, C.byref(p), None, C.c_uint32(1), out) == 1
    assert L.zk_verify_batch(verifier._h, C.byref(p), zk._p64(i), C.c_uint32(1), None) == 1
    assert L.zk_verify_batch_json(None, arr, C.c_uint32(1), out) == 1
    assert L.zk_verify_batch_json(verifier._h, None, C.c_uint32(1), out) == 1
    assert L.zk_verify_batch_json(verifier._h, arr, C.c_uint32(1), None) == 1
    assert L.zk_verify_batch_json(verifier._h, (C.c_char_p * 1)(None), C.c_uint32(1), out) == 1
    h = C.c_void_p()
    vk = zk.vk_from_json(vkj)
    assert L.zk_vctx_create(None, 0, C.c_uint32(1), C.byref(h)) == 1
    assert L.zk_vctx_create(vk._h, 0, C.c_uint32(0), C.byref(h)) == 1
    assert L.zk_vctx_create(vk._h, 0, C.c_uint32(1), None) == 1
    assert L.zk_vctx_create(vk._h, 99, C.c_uint32(1), C.byref(h)) == 1
    L.zk_vctx_destroy(None)
    # a key with a point off its curve
    d = json.loads(vkj)
    d["gamma"][0][0] = "0x5"
    with pytest.raises(zk.ZkError) as e:
        zk.Verifier(json.dumps(d))
    assert e.value.code == 3
    d = json.loads(vkj)
    d["gammaABC"][1][1] = "0x5"
    with pytest.raises(zk.ZkError) as e:
        zk.Verifier(json.dumps(d))
    assert e.value.code == 3
    assert verifier.verify([valid, bad]) == [True, False]                               # the context is still good
    verifier.close()


def test_reference_static_triple(zk):
    d = json.load(open(os.path.join(GOLDEN, "ref_static_triple.json")))
    vkj = json.dumps(d["vk"])
    valid = json.dumps(d["proof"])
    t1 = json.dumps(dict(d["proof"], input=[d["proof"]["input"][0], "0x8"]))
    t2 = json.dumps(dict(d["proof"], A=d["proof"]["C"]))
    t3 = json.dumps(dict(d["proof"], input=d["proof"]["input"][:1]))
    texts = [t1, valid, t2, t3, valid]
    verifier = zk.Verifier(vkj, max_batch=8)
    assert verifier.verify(texts) == V.expected(zk, vkj, texts) == [False, True, False, False, True]
    verifier.close()


@pytest.mark.parametrize("nIn", [0, 1, 2, 3])
def test_input_counts_tables_and_fallback(zk, nIn, monkeypatch):
    """keys with 0 .. 3 inputs: the accumulation from the window tables and, with a table budget of one byte, by double-and-add"""
    nC = 12
    r, w = R.random_r1cs(nC, nIn, seed=60 + nIn)
    _, w2 = R.random_r1cs(nC, nIn, seed=60 + nIn, witness_seed=71)
    toxic = [R.SplitMix64(17 + nIn).fr() for _ in range(5)]
    pk, vk = zk.keygen(r, toxic=toxic)
    ctx = zk.ProverContext(pk, r)
    p1, p2 = zk.prove(ctx, F.fr_to_mont(w)), zk.prove(ctx, F.fr_to_mont(w2))
    ctx.close()
    vkj = vk.to_json()
    texts = [p1, V.tamper_pairing("input", p1), p2, V.tamper_pairing("C+G", p2)]
    if nIn:
        texts += list(V.swap_inputs(p1, p2))
        edge = V.parse(p1)                                                              # inputs 0 and r - 1 are in range
        texts += [V.text(edge[0], edge[1], edge[2], [0] * nIn), V.text(edge[0], edge[1], edge[2], [pyref.R - 1] * nIn)]
    want = V.expected(zk, vkj, texts)
    assert want[:4] == [True, False, True, False] and not any(want[4:])
    assert pyref.verify(json.loads(vkj), V.as_dict(p1)) and not pyref.verify(json.loads(vkj), V.as_dict(texts[1]))
    verifier = zk.Verifier(vk, max_batch=len(texts))
    assert verifier.verify(texts) == want
    verifier.close()
    monkeypatch.setenv("ZK_VERIFY_TABLE_BUDGET", "1")
    verifier = zk.Verifier(vk, max_batch=len(texts))
    monkeypatch.delenv("ZK_VERIFY_TABLE_BUDGET")
    assert verifier.verify(texts) == want
    verifier.close()


def test_new_entry_points_end_in_the_exception_barrier():
    """the scan of test_abi.py for the new unit: every extern "C" function that returns a code is a function-try-block ending in ZK_GUARD*"""
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "ethsnarks_amd", "csrc", "verify_gpu.cpp")).read()
    src = "\n".join(l for l in src.split("\n") if not l.lstrip().startswith("//"))     # (a comment between two functions is no function body)
    heads = list(re.finditer(r'^extern "C" [^\n;]*?(\w+)\s*\(([^;{]*?)\)\s*(try\s*)?\{', src, flags=re.M))
    assert len(heads) == 9
    for i, m in enumerate(heads):
        body = src[m.end():heads[i + 1].start() if i + 1 < len(heads) else len(src)]
        assert m.group(3), m.group(1) + " is not a function-try-block"
        assert re.search(r"\}\s*ZK_GUARD(_VOID|_BOOL)?\s*$", body.strip()), m.group(1) + " does not end in ZK_GUARD"
    hdr = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for m in heads:
        assert re.search(r"\b%s\s*\(" % m.group(1), hdr), m.group(1) + " is not declared in zkhip.h"


def test_cpp_adapter_verify_batch(emul, emul_verify, tmp_path):
    """stub_verify_batch of include/ethsnarks_hip/stubs.hpp, compiled with g++ -Werror and run against the emulation build"""
    from conftest import ROOT
    exe = str(tmp_path / "verify_batch_test")
    d, dv = os.path.dirname(emul), os.path.dirname(emul_verify)
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "verify_batch_test.cpp"), "-o", exe, "-L" + dv, "-lzkhip_emul_verify", "-L" + d, "-lzkhip_emul",
                        "-Wl,-rpath," + dv, "-Wl,-rpath," + d],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    case = golden_cases()[0]
    vkf, pf, bf = tmp_path / "vk.json", tmp_path / "proof.json", tmp_path / "bad.json"
    vkf.write_text(json.dumps(case["vk"])); pf.write_text(case["proof_json"]); bf.write_text(V.tamper_pairing("A2", case["proof_json"]))
    p = subprocess.run([exe, str(vkf), str(pf), str(bf)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "BATCH OK", p.stdout + p.stderr
