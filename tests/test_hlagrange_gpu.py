"""The four-transform prover (H-query in coset-Lagrange bases) on the device: proof bytes against the six-transform path
(ZK_SIX_TRANSFORMS=1, read at context creation) and against the oracle, the degree check on both paths, and the sharing of the tables.
Domains: 2^3 (the smallest the chain circuit gives), 2^10 (one transform pass), 2^12 (two passes)."""
import numpy as np
import pytest
from ethsnarks_amd import r1cs as R, fields as F, gadgets as G
import zk_closed_form as Z

pytestmark = pytest.mark.gpu


def _contexts(hip, monkeypatch, pk, r, **kw):
    four = hip.ProverContext(pk, r, **kw)
    monkeypatch.setenv("ZK_SIX_TRANSFORMS", "1")
    six = hip.ProverContext(pk, r, **kw)
    monkeypatch.delenv("ZK_SIX_TRANSFORMS")
    assert four.info()["four_transforms"] and not six.info()["four_transforms"]
    return four, six


@pytest.mark.parametrize("nC,nIn", [(6, 1), (4, 3), (1022, 1), (1020, 3), (4094, 1)])
def test_chain_proof_bytes(hip, oracle, monkeypatch, nC, nIn):
    r, w = R.synthetic_chain(nC, nIn)
    wm = F.fr_to_mont(w)
    pk_o, _ = oracle.keygen(r, seed=nC + nIn)
    expect, _ = oracle.prove(pk_o, r, wm)
    pk = hip.ProvingKey.from_parts(**pk_o.parts())
    four, six = _contexts(hip, monkeypatch, pk, r)
    assert hip.prove(four, wm) == expect
    assert hip.prove(six, wm) == expect
    i4, i6 = four.info(), six.info()
    # the tables hold m and V + 1 bases where the key's own hold m - 1 and V - nIn: m + nIn + 1 bases more, each with its window's rows
    m, V = r.domain_size, r.V
    assert i4["table_bytes"] - i6["table_bytes"] == 64 * (i4["H"]["W"] * m + i4["L"]["W"] * (V + 1) - i6["H"]["W"] * (m - 1) - i6["L"]["W"] * (V - nIn))
    # an unsatisfying witness is refused by both paths with the same code (ZK_ERR_DEGREE = 7)
    bad = list(w); bad[len(bad) // 2] = (bad[len(bad) // 2] + 1) % F.FR
    for ctx in (four, six):
        with pytest.raises(hip.ZkError) as e:
            hip.prove(ctx, F.fr_to_mont(bad))
        assert e.value.code == 7
        assert hip.prove(ctx, wm) == expect                               # ... and the context proves on
    four.close(); six.close(); pk.close()


def test_mimc_preimage_proof_bytes(hip, oracle, monkeypatch):
    r, w, _ = G.mimc_preimage_circuit(11)                                # 4 015 constraints: domain 2^12
    wm = F.fr_to_mont(w)
    pk_o, _ = oracle.keygen(r, seed=12)
    expect, _ = oracle.prove(pk_o, r, wm)
    pk = hip.ProvingKey.from_parts(**pk_o.parts())
    four, six = _contexts(hip, monkeypatch, pk, r)
    assert hip.prove(four, wm) == expect
    assert hip.prove(six, wm) == expect
    four.close(); six.close(); pk.close()


def test_batch_of_three_and_zero_knowledge(hip, monkeypatch):
    """three distinct witnesses through one launch sequence, and zero-knowledge proofs with fixed (r, s): both paths against the closed
    form of the proof in the trapdoor (zk_closed_form.py; r = s = 0 is the proof without blinding)"""
    r, w0 = R.random_r1cs(300, 2, seed=21)
    ws = [w0] + [R.random_r1cs(300, 2, seed=21, witness_seed=s)[1] for s in (5, 6)]
    wm = np.stack([F.fr_to_mont(w) for w in ws])
    toxic = [0x1234567 + 11 * i for i in range(5)]
    pk, _ = hip.keygen(r, toxic=toxic, full=True)
    four, six = _contexts(hip, monkeypatch, pk, r, max_batch=3)
    rp = r.as_pyref()
    sums = [Z.trapdoor_sums(rp, w, *toxic) for w in ws]
    plain = [Z.zk_proof_json(rp, w, toxic, 0, 0, s) for w, s in zip(ws, sums)]
    assert len(set(plain)) == 3
    rs = (0x1234567, 0x89abcdef)
    blind = [Z.zk_proof_json(rp, w, toxic, rs[0], rs[1], s) for w, s in zip(ws, sums)]
    for ctx in (four, six):
        assert hip.prove_batch(ctx, wm) == plain
        assert [hip.prove(ctx, wm[i]) for i in range(3)] == plain
        assert ctx.prove_zk(wm[0], rs=rs) == blind[0]
        assert ctx.prove_zk_batch(wm, rs=[rs] * 3) == blind
    four.close(); six.close(); pk.close()


def test_two_step_submit_on_a_four_transform_context(hip, oracle):
    """h handed over as coefficients (zk_prove_submit_defer_h, the three chains, zk_h_from_chains_submit, zk_prove_submit_h) on an unsharded
    context with default settings: the coefficients go to the coset (two transforms) and meet the Lagrange bases there"""
    r, w = R.random_r1cs(1000, 2, seed=15)
    wm = F.fr_to_mont(w)
    pk_o, _ = oracle.keygen(r, seed=9)
    expect = oracle.prove(pk_o, r, wm)[0]
    pk = hip.ProvingKey.from_parts(**pk_o.parts())
    c = hip.ProverContext(pk, r)
    assert c.info()["four_transforms"]
    c.submit_defer_h(wm)
    for which in range(3):
        c.chain_submit(None, which)
    c.chain_wait()
    c.h_from_chains_submit(c.chain_device_ptr(0), c.chain_device_ptr(1), c.chain_device_ptr(2))
    c.chain_wait(check_degree=True)
    c.submit_h(c.h_device_ptr())
    part, _ = c.collect()
    assert hip.proof_to_json(c.prove_combine(part), wm[1:3]) == expect
    assert hip.prove(c, wm) == expect
    c.close(); pk.close()


def test_tables_are_built_once_per_key_and_circuit(hip, oracle):
    r, w = R.synthetic_chain(1022, 1)
    wm = F.fr_to_mont(w)
    pk_o, _ = oracle.keygen(r, seed=8)
    expect, _ = oracle.prove(pk_o, r, wm)
    pk = hip.ProvingKey.from_parts(**pk_o.parts())
    n0 = hip.launch_count(); a = hip.ProverContext(pk, r); n1 = hip.launch_count(); b = hip.ProverContext(pk, r); n2 = hip.launch_count()
    assert n1 - n0 > 2 * 10                                              # the first context ran the two group transforms (10 stages each) ...
    assert n2 - n1 < 16                                                  # ... the second only filled its own transform tables
    assert a.info()["hlagrange_precompute_ms"] == b.info()["hlagrange_precompute_ms"] > 0
    assert hip.prove(a, wm) == hip.prove(b, wm) == expect
    a.close(); b.close(); pk.close()
