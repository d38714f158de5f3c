"""What test_eddsa_pure_emul.py and test_eddsa_pure_gpu.py share: EdDSAVerifier("pure").fill_pedersen_witnesses against the front end's witness
element by element, the verdicts against zk_eddsa_verify_batch and jubjub_cases.verify, sentinels in untouched rows and guard elements, the
refusals, and the chain circuit -> keygen -> fill -> submit_batch(device_ptr=...) -> proofs."""
import ctypes as C
import json

import numpy as np

from ethsnarks_amd import fields as F
from ethsnarks_amd.fields import FR
import eddsa_pure_cases as PC
import jubjub_cases as JC

GUARD = 1                                                              # elements between the rows that no fill may touch


def sentinel(rows, elems):
    return np.arange(4 * elems * rows, dtype=np.uint64).reshape(rows, elems, 4) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(7)


def fill(zk, v, items, row_elems):
    """(sentinel, buffer afterwards, verdicts) over len(items) + 1 rows"""
    n = len(items)
    s = sentinel(n + 1, row_elems)
    buf = zk.DeviceBuffer(32 * row_elems * (n + 1))
    buf.upload(s)
    verdicts, _ = v.fill_pedersen_witnesses([c[1] for c in items], [c[2] for c in items], [c[3] for c in items], buf, row_elems=row_elems)
    got = buf.download((n + 1, row_elems, 4))
    buf.free()
    return s, got, verdicts


def check_items(zk, J, items, msg_len, B=None, satisfied=True):
    """every well-formed item's row equals the front end's witness as field elements (canonical Montgomery limbs), its verdict the
    restatement's and the batch verifier's; a malformed item's row, the guard element of every row and the row after the last keep the sentinel"""
    n = len(items)
    with J.EdDSAVerifier("pure", B=B, msg_len=msg_len) as v:
        r, lay = v.pedersen_circuit()
        elems = lay.n_vars + 1
        assert r.V == lay.n_vars and r.nIn == 2 + 8 * msg_len
        s, got, verdicts = fill(zk, v, items, elems + GUARD)
        assert np.array_equal(got[:, elems:], s[:, elems:]) and np.array_equal(got[n], s[n])
        full = 0
        for i, item in enumerate(items):
            label, A, (R, sv), msg, want = item
            assert verdicts[i] == want == JC.verify("pure", A, (R, sv), msg, B or JC.GENERATOR), (i, label)
            if label in PC.MALFORMED:
                assert np.array_equal(got[i], s[i]), (i, label)
                continue
            w = PC.expected_row(v._pedersen_circuit, item)
            assert np.array_equal(got[i, :elems], F.fr_to_mont(w)), (i, label, np.flatnonzero((got[i, :elems] != F.fr_to_mont(w)).any(axis=1))[:8])
            if satisfied:
                assert v._pedersen_circuit.r1cs().is_satisfied(w) == (want and R not in JC.LOW_ORDER), (i, label)
            full += 1
        ok = [i for i, c in enumerate(items) if c[2][1] < FR]          # zk_eddsa_verify_batch refuses a batch that holds an s >= r
        batch = v.verify([items[i][1] for i in ok], [items[i][2] for i in ok], [items[i][3] for i in ok])
        assert batch == [verdicts[i] for i in ok]
        assert full >= 1 and (n < 64 or (full < n and not all(verdicts) and any(verdicts)))
    return items


def check_rows(zk, J, n, msg_len=1, B=None):
    return check_items(zk, J, PC.batch(n, msg_len, B or JC.GENERATOR), msg_len, B, satisfied=n <= 3)


def check_one_shot_iterables(J):
    """fill_pedersen_witnesses reads sigs (any iterable, a zip or a generator included) exactly once, as verify does"""
    items = [c for c in PC.batch(3) if c[0] not in PC.MALFORMED]
    A, sigs, msgs, want = [c[1] for c in items], [c[2] for c in items], [c[3] for c in items], [c[4] for c in items]
    with J.EdDSAVerifier("pure", msg_len=1) as v:
        verdicts, buf = v.fill_pedersen_witnesses(iter(A), zip([R for R, _ in sigs], [s for _, s in sigs]), (m for m in msgs))
        assert verdicts == want
        buf.free()


def check_refusals(zk, J):
    """ZK_ERR_ARG (1) and an untouched buffer: another scheme, a row one element short, the layout of another msg_len, a layout whose segments
    collide, leave the row or touch variable 0, a coordinate >= r; then n = 0 and the Python errors"""
    item = PC.batch(1)[0]
    lib = zk._lib
    pts = lambda p: F.ints_to_limbs(list(p))
    with J.EdDSAVerifier("pure", msg_len=1) as v, J.EdDSAVerifier("mimc", msg_len=1) as mimc, J.EdDSAVerifier("hash", msg_len=1) as hsh, \
            J.EdDSAVerifier("pure", msg_len=2) as v2:
        _, lay = v.pedersen_circuit()
        _, lay2 = v2.pedersen_circuit()
        elems = lay.n_vars + 1
        s = sentinel(2, elems)
        buf = zk.DeviceBuffer(s.nbytes)
        buf.upload(s)

        def call(handle, layout, row_elems, A=item[1], R=item[2][0], sv=item[2][1], msg=item[3]):
            arrs = [pts(A), pts(R), F.ints_to_limbs([sv]), np.frombuffer(bytes(msg) + b"\0" * 8, dtype=np.uint8).copy()]
            out = np.full(1, 7, dtype=np.uint8)
            rc = lib.zk_eddsa_fill_pure_witnesses(handle, *[a.ctypes.data_as(C.c_void_p) for a in arrs], 1, C.c_void_p(buf.ptr), C.c_uint64(row_elems),
                                                  C.byref(J.EddsaPureLayout(*layout)), out.ctypes.data_as(C.c_void_p))
            assert rc == 0 or (out[0] == 7 and np.array_equal(buf.download(s.shape), s)), "a refused call wrote something"
            return rc

        assert call(mimc._h, lay, elems) == 1 and call(hsh._h, lay, elems) == 1        # the scheme
        assert call(v._h, lay, elems - 1) == 1                                         # a short row
        assert call(v._h, lay2, lay2.n_vars + 1) == 1 and call(v2._h, lay, elems) == 1  # another msg_len
        assert call(v._h, lay._replace(msg_len=2), elems) == 1
        assert call(v._h, lay._replace(last_adder_var0=lay.last_adder_var0 + 1), elems) == 1        # leaves the row
        assert call(v._h, lay._replace(n_vars=lay.n_vars + 1), elems) == 1
        assert call(v._h, lay._replace(t_range_var0=lay.t_range_var0 - 1), elems) == 1              # overlaps the comparisons
        assert call(v._h, lay._replace(converter_var0=lay.converter_var0 - 1), elems) == 1          # overlaps the last Montgomery adder
        assert call(v._h, lay._replace(edwards_adder_var0=lay.edwards_adder_var0 + 1), elems) == 1  # runs into the bits of t
        assert call(v._h, lay._replace(hash_window_var0=lay.ax_range_var0 + 98), elems) == 1
        assert call(v._h, lay._replace(step_stride=14), elems) == 1 and call(v._h, lay._replace(cond_var0=lay.doubler_var0 + 5), elems) == 1
        assert call(v._h, lay._replace(ax_var=0), elems) == 1                                       # variable 0 is ONE
        assert call(v._h, lay._replace(window_var0=0xFFFFFF00), elems) == 1
        assert call(v._h, lay, elems, A=(FR, 1)) == 1 and call(v._h, lay, elems, R=(0, FR)) == 1
        assert lib.zk_eddsa_fill_pure_witnesses(v._h, None, None, None, None, 1, None, C.c_uint64(elems), None, None) == 1
        assert call(v._h, lay, elems) == 0                                             # and the same call with nothing wrong fills row 0
        got = buf.download(s.shape)
        assert np.array_equal(got[0], F.fr_to_mont(PC.expected_row(v._pedersen_circuit, item))) and np.array_equal(got[1], s[1])
        assert v.fill_pedersen_witnesses([], [], [], buf)[0] == []
        mitem = JC.signature_cases("mimc", 1)[0]
        for fn in (mimc.pedersen_circuit, hsh.pedersen_circuit, lambda: mimc.fill_pedersen_witnesses([mitem[1]], [mitem[2]], [mitem[3]], buf),
                   lambda: hsh.fill_pedersen_witnesses([item[1]], [item[2]], [item[3]], buf)):
            try:
                fn()
                raise AssertionError("a scheme without a Pedersen circuit was accepted")
            except NotImplementedError:
                pass
        for fn in (lambda: v.fill_pedersen_witnesses([item[1]] * 3, [item[2]] * 3, [item[3]] * 3, buf),      # a buffer of two rows
                   lambda: v.fill_pedersen_witnesses([item[1]], [item[2]], [b"ab"], buf)):                   # two bytes for msg_len 1
            try:
                fn()
                raise AssertionError("a call that cannot be right was accepted")
            except ValueError:
                pass
        buf.free()


def check_proofs(zk, J, items, accept, seed=43):
    """keygen on the circuit, the rows filled on the device, submit_batch(device_ptr=...).  The prover refuses a batch that holds the row of a
    wrong signature (ZK_ERR_DEGREE = 7) and goes on working; the items whose verdict is 1 are then filled side by side into a second buffer and
    proven in ONE submit of that many rows.  Returns the key and one proof text per item under the item's OWN public inputs: for a refused item
    the text of an accepted item's proof with the refused item's inputs, which is all a holder of a wrong signature can present"""
    k = len(items)
    with J.EdDSAVerifier("pure", msg_len=len(items[0][3])) as v:
        r, lay = v.pedersen_circuit()
        pk, vk = zk.keygen(r, seed=seed)
        verdicts, buf = v.fill_pedersen_witnesses([c[1] for c in items], [c[2] for c in items], [c[3] for c in items])
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
            again, rows = v.fill_pedersen_witnesses([items[p][1] for p in good], [items[p][2] for p in good], [items[p][3] for p in good])
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
            assert [int(x, 16) for x in json.loads(texts[p])["input"]] == v._pedersen_circuit.public_inputs(item[1], item[3])
        ctx.close(); buf.free()
    return vk, texts
