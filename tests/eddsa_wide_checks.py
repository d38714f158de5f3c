"""What test_eddsa_wide_emul.py and test_eddsa_wide_gpu.py share: EdDSAVerifier.fill_witnesses(lanes=2 or 4) -- zk_eddsa_fill_witnesses_wide,
csrc/jubjub.hpp k_eddsa_fill_wide -- held to what eddsa_circuit_checks.py holds the one-lane fill to.  Expected rows are the front end's own
witness (eddsa_circuit_cases.expected_row), expected verdicts jubjub_cases.verify on Python integers; never a kernel's output, except where a
test says that two fills must leave the same bytes."""
import ctypes as C
import json

import numpy as np

from ethsnarks_amd import fields as F
from ethsnarks_amd.fields import FR
import eddsa_circuit_cases as EC
import eddsa_circuit_checks as narrow
import jubjub_cases as JC

GUARD = narrow.GUARD
WIDE = (2, 4)


def fill(zk, v, items, row_elems, lanes):
    """(sentinel, buffer afterwards, verdicts) over len(items) + 1 rows"""
    n = len(items)
    s = narrow.sentinel(n + 1, row_elems)
    buf = zk.DeviceBuffer(32 * row_elems * (n + 1))
    buf.upload(s)
    verdicts, _ = v.fill_witnesses([c[1] for c in items], [c[2] for c in items], [c[3] for c in items], buf, row_elems=row_elems, lanes=lanes)
    got = buf.download((n + 1, row_elems, 4))
    buf.free()
    return s, got, verdicts


def check_rows(zk, J, n, lanes, msg_len=1, B=None):
    """eddsa_circuit_checks.check_rows with `lanes` lanes per signature: every well-formed item's row equals the front end's witness element for
    element, its verdict the restatement's and the batch verifier's; a malformed item's row, the guard element of every row and the row after
    the last keep the sentinel.  Returns the buffer"""
    items = EC.batch(n, msg_len, B or JC.GENERATOR)
    with J.EdDSAVerifier("mimc", B=B, msg_len=msg_len) as v:
        r, lay = v.circuit()
        elems = lay.n_vars + 1
        s, got, verdicts = fill(zk, v, items, elems + GUARD, lanes)
        assert np.array_equal(got[:, elems:], s[:, elems:]) and np.array_equal(got[n], s[n])
        full = 0
        for i, item in enumerate(items):
            label, A, (R, sv), msg, want = item
            assert verdicts[i] == want == JC.verify("mimc", A, (R, sv), msg, B or JC.GENERATOR), (i, label)
            if label in EC.MALFORMED:
                assert np.array_equal(got[i], s[i]), (i, label)
                continue
            row = EC.expected_row(v._circuit, item)
            w = F.fr_to_mont(row)
            assert np.array_equal(got[i, :elems], w), (i, label, np.flatnonzero((got[i, :elems] != w).any(axis=1))[:8])
            assert v._circuit.r1cs().is_satisfied(row) == (want and R not in JC.LOW_ORDER) or n > 3, (i, label)
            full += 1
        ok = [i for i, c in enumerate(items) if c[2][1] < FR]          # zk_eddsa_verify_batch refuses a batch that holds an s >= r
        batch = v.verify([items[i][1] for i in ok], [items[i][2] for i in ok], [items[i][3] for i in ok])
        assert batch == [verdicts[i] for i in ok]
        assert full >= 1 and (n < 64 or (full < n and not all(verdicts) and any(verdicts)))
    return got


def check_dead_workgroup(zk, J, lanes):
    """two items, both malformed: no lane of the workgroup has a witness to fill.  The call completes, answers 0, 0 and writes nothing"""
    by = {c[0]: c for c in EC.directed(1)}
    items = [by["off-curve A"], by["s = 2^254"]]
    with J.EdDSAVerifier("mimc", msg_len=1) as v:
        _, lay = v.circuit()
        s, got, verdicts = fill(zk, v, items, lay.n_vars + 1 + GUARD, lanes)
    assert verdicts == [False, False]
    assert np.array_equal(got, s)


def check_same_bytes_as_one_lane(zk, J, n=65):
    """the buffer after lanes = 2 and after lanes = 4 is the buffer after lanes = 1, guards, malformed rows and the row after the last included"""
    items = EC.batch(n)
    with J.EdDSAVerifier("mimc", msg_len=1) as v:
        _, lay = v.circuit()
        _, one, verdicts = fill(zk, v, items, lay.n_vars + 1 + GUARD, 1)
        for lanes in WIDE:
            _, got, again = fill(zk, v, items, lay.n_vars + 1 + GUARD, lanes)
            assert again == verdicts, lanes
            assert got.tobytes() == one.tobytes(), (lanes, np.flatnonzero((got != one).any(axis=(1, 2)))[:8])


def check_refusals(zk, J):
    """lanes outside (1, 2, 4): ZK_ERR_ARG (1) through the C entry and a ValueError in Python; with lanes = 2 and 4 the refusals of the narrow
    entry -- another scheme, a short row, a null layout; each with the buffer and the verdict untouched.  Then the same call with nothing
    wrong fills row 0"""
    item = EC.batch(1)[0]
    lib = J._wide_fill_lib()
    pts = lambda p: F.ints_to_limbs(list(p))
    with J.EdDSAVerifier("mimc", msg_len=1) as v, J.EdDSAVerifier("pure", msg_len=1) as pure:
        _, lay = v.circuit()
        elems = lay.n_vars + 1
        s = narrow.sentinel(2, elems)
        buf = zk.DeviceBuffer(s.nbytes)
        buf.upload(s)

        def call(handle, layout, row_elems, lanes):
            arrs = [pts(item[1]), pts(item[2][0]), F.ints_to_limbs([item[2][1]]), F.ints_to_limbs(list(item[3]))]
            out = np.full(1, 7, dtype=np.uint8)
            rc = lib.zk_eddsa_fill_witnesses_wide(handle, *[a.ctypes.data_as(C.c_void_p) for a in arrs], 1, C.c_void_p(buf.ptr), C.c_uint64(row_elems),
                                                  C.byref(J.EddsaLayout(*layout)) if layout is not None else None, out.ctypes.data_as(C.c_void_p), lanes)
            assert rc == 0 or (out[0] == 7 and np.array_equal(buf.download(s.shape), s)), "a refused call wrote something"
            return rc

        for lanes in (0, 3, 8):
            assert call(v._h, lay, elems, lanes) == 1
            try:
                v.fill_witnesses([item[1]], [item[2]], [item[3]], buf, lanes=lanes)
                raise AssertionError("lanes = %d was accepted" % lanes)
            except ValueError:
                pass
        for lanes in (1,) + WIDE:
            assert call(pure._h, lay, elems, lanes) == 1                               # the scheme
            assert call(v._h, lay, elems - 1, lanes) == 1                              # a short row
            assert call(v._h, None, elems, lanes) == 1                                 # a null layout
            assert call(v._h, lay._replace(msg_len=3), elems, lanes) == 1
        assert np.array_equal(buf.download(s.shape), s)
        w = F.fr_to_mont(EC.expected_row(v._circuit, item))
        for lanes in WIDE:
            buf.upload(s)
            assert call(v._h, lay, elems, lanes) == 0
            got = buf.download(s.shape)
            assert np.array_equal(got[0], w) and np.array_equal(got[1], s[1])
            assert v.fill_witnesses([], [], [], buf, lanes=lanes)[0] == []
        try:
            pure.fill_witnesses([item[1]], [item[2]], [b"a"], buf, lanes=4)
            raise AssertionError("a scheme without a circuit was accepted")
        except NotImplementedError:
            pass
        buf.free()


def check_proofs(zk, J, items, accept, lanes, seed=41):
    """eddsa_circuit_checks.check_proofs, whose fill is EdDSAVerifier.fill_witnesses without arguments, restated step for step with
    fill_witnesses(lanes=lanes): keygen on the circuit, the rows filled on the device, submit_batch(device_ptr=...); the prover refuses the
    batch that holds a wrong signature's row (ZK_ERR_DEGREE = 7) and goes on working; the items whose verdict is 1 are filled side by side into
    a second buffer and proven in one submit.  Returns the key and one proof text per item under the item's own public inputs"""
    k = len(items)
    with J.EdDSAVerifier("mimc", msg_len=len(items[0][3])) as v:
        r, lay = v.circuit()
        pk, vk = zk.keygen(r, seed=seed)
        verdicts, buf = v.fill_witnesses([c[1] for c in items], [c[2] for c in items], [c[3] for c in items], lanes=lanes)
        assert verdicts == [c[4] for c in items] == accept and any(accept)
        ctx = zk.ProverContext(pk, r, max_batch=k)
        if not all(accept):
            ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
            try:
                ctx.collect_batch(k)
                raise AssertionError("a batch with the row of a wrong signature was proven")
            except zk.ZkError as e:
                assert e.code == 7
        w = buf.download((k, r.V + 1, 4))
        good = [p for p in range(k) if accept[p]]
        if len(good) < k:
            again, rows = v.fill_witnesses([items[p][1] for p in good], [items[p][2] for p in good], [items[p][3] for p in good], lanes=lanes)
            assert again == [True] * len(good)
            assert np.array_equal(rows.download((len(good), r.V + 1, 4)), w[good])
        else:
            rows = buf
        ctx.submit_batch(None, device_ptr=rows.ptr, k=len(good))
        parts, _ = ctx.collect_batch(len(good))
        proofs = {p: ctx.prove_combine(parts[j]) for j, p in enumerate(good)}
        if rows is not buf:
            rows.free()
        stand_in = proofs[good[0]]
        texts = [zk.proof_to_json(proofs.get(p, stand_in), w[p][1:1 + r.nIn]) for p in range(k)]
        for p, item in enumerate(items):
            assert [int(x, 16) for x in json.loads(texts[p])["input"]] == v._circuit.public_inputs(item[1], item[3])
        ctx.close(); buf.free()
    return vk, texts
