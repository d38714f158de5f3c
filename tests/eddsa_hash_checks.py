"""What test_eddsa_hash_emul.py and test_eddsa_hash_gpu.py share: EdDSAVerifier("hash").fill_hash_witnesses against the front end's witness
element by element, the verdicts against zk_eddsa_verify_batch and jubjub_cases.verify, sentinels in untouched rows and guard elements, the
refusals, and the chain EdDSASigner -> circuit -> keygen -> fill -> submit_batch(device_ptr=...) -> proofs."""
import ctypes as C
import json

import numpy as np

from ethsnarks_amd import fields as F
from ethsnarks_amd.fields import FR
from eddsa_pure_checks import GUARD, sentinel
import eddsa_hash_cases as HC
import jubjub_cases as JC


def fill(zk, v, items, row_elems):
    """(sentinel, buffer afterwards, verdicts) over len(items) + 1 rows"""
    n = len(items)
    s = sentinel(n + 1, row_elems)
    buf = zk.DeviceBuffer(32 * row_elems * (n + 1))
    buf.upload(s)
    verdicts, _ = v.fill_hash_witnesses([c[1] for c in items], [c[2] for c in items], [c[3] for c in items], buf, row_elems=row_elems)
    got = buf.download((n + 1, row_elems, 4))
    buf.free()
    return s, got, verdicts


def check_items(zk, J, items, msg_len, B=None, satisfied=True):
    """every well-formed item's row equals the front end's witness as field elements (canonical Montgomery limbs), its verdict the
    restatement's and the batch verifier's; a malformed item's row, the guard element of every row and the row after the last keep the sentinel"""
    n = len(items)
    with J.EdDSAVerifier("hash", B=B, msg_len=msg_len) as v:
        r, lay = v.hash_circuit()
        elems = lay.n_vars + 1
        assert r.V == lay.n_vars and r.nIn == 2 + 8 * msg_len and lay.msg_len == msg_len
        s, got, verdicts = fill(zk, v, items, elems + GUARD)
        assert np.array_equal(got[:, elems:], s[:, elems:]) and np.array_equal(got[n], s[n])
        full = 0
        for i, item in enumerate(items):
            label, A, (R, sv), msg, want = item
            assert verdicts[i] == want == JC.verify("hash", A, (R, sv), msg, B or JC.GENERATOR), (i, label)
            if label in HC.MALFORMED:
                assert np.array_equal(got[i], s[i]), (i, label)
                continue
            w = HC.expected_row(v._hash_circuit, item)
            assert np.array_equal(got[i, :elems], F.fr_to_mont(w)), (i, label, np.flatnonzero((got[i, :elems] != F.fr_to_mont(w)).any(axis=1))[:8])
            if satisfied:
                assert v._hash_circuit.r1cs().is_satisfied(w) == (want and R not in JC.LOW_ORDER), (i, label)
            full += 1
        ok = [i for i, c in enumerate(items) if c[2][1] < FR]          # zk_eddsa_verify_batch refuses a batch that holds an s >= r
        batch = v.verify([items[i][1] for i in ok], [items[i][2] for i in ok], [items[i][3] for i in ok])
        assert batch == [verdicts[i] for i in ok]
        assert full >= 1 and (n < 64 or (full < n and not all(verdicts) and any(verdicts)))
    return items


def check_rows(zk, J, n, msg_len=1, B=None):
    return check_items(zk, J, HC.batch(n, msg_len, B or JC.GENERATOR), msg_len, B, satisfied=n <= 3)


def check_layout_shape(J, msg_len, pad, segments, lone):
    """the message hash's segments as the layout places them: empty ones take no room, the lone window's converter stands first"""
    c = J.JG.EddsaHashCircuit(msg_len)
    lay, fb, W = c.layout, c.msg_hashed.hash.commitment, HC.msg_windows(msg_len)
    assert len(c.pad_bits) == pad == lay.m_window_var0 - lay.m_pad_bit0 and lay.m_mont_adder_var0 - lay.m_window_var0 == 2 * W
    assert len(fb.point_converters) == segments and lay.m_converter_var0 - lay.m_mont_adder_var0 == 3 * (W - segments)
    assert lay.m_edwards_adder_var0 - lay.m_converter_var0 == 2 * segments and lay.m_bit0 - lay.m_edwards_adder_var0 == 7 * (segments - 1)
    assert lay.m_range_var0 - lay.m_bit0 == 3 * 254 - 1 and lay.validator_var0 - lay.m_range_var0 == 99
    assert (fb.point_converters[0].y1 == fb.windows_y[-1].result()) == lone
    assert c.core.hash.hash.commitment.n_windows == 254 and len(c.core.hash.hash.commitment.point_converters) == 5
    assert tuple(J.JG.eddsa_hash_circuit(msg_len)[1]) == tuple(lay)


def check_one_shot_iterables(J):
    """fill_hash_witnesses reads sigs (any iterable, a zip or a generator included) exactly once, as verify does"""
    items = [c for c in HC.batch(3) if c[0] not in HC.MALFORMED]
    A, sigs, msgs, want = [c[1] for c in items], [c[2] for c in items], [c[3] for c in items], [c[4] for c in items]
    with J.EdDSAVerifier("hash", msg_len=1) as v:
        verdicts, buf = v.fill_hash_witnesses(iter(A), zip([R for R, _ in sigs], [s for _, s in sigs]), (m for m in msgs))
        assert verdicts == want
        buf.free()


def check_refusals(zk, J):
    """ZK_ERR_ARG (1) and an untouched buffer: another scheme, a row one element short, the layout of another msg_len, a layout whose segments
    collide, leave the row or touch variable 0 -- every segment of the message hash in turn -- a coordinate >= r, nulls; an EMPTY segment's
    offset is not looked at; then n = 0 and the Python errors"""
    item, item24 = HC.batch(1)[0], HC.one_valid(HC.TWO_SEGMENT_MSG_LEN)
    lib = zk._lib
    assert zk.ABI_VERSION == 9 and lib.zk_abi_version() == 9 and "zk_eddsa_fill_hash_witnesses" in zk.EXPORTS
    pts = lambda p: F.ints_to_limbs(list(p))
    with J.EdDSAVerifier("hash", msg_len=1) as v, J.EdDSAVerifier("mimc", msg_len=1) as mimc, J.EdDSAVerifier("pure", msg_len=1) as pure, \
            J.EdDSAVerifier("hash", msg_len=3) as v3, J.EdDSAVerifier("hash", msg_len=HC.TWO_SEGMENT_MSG_LEN) as v24:
        (_, lay), (_, lay3), (_, lay24) = v.hash_circuit(), v3.hash_circuit(), v24.hash_circuit()
        elems, elems24 = lay.n_vars + 1, lay24.n_vars + 1
        s = sentinel(2, elems24)
        buf = zk.DeviceBuffer(s.nbytes)
        buf.upload(s)

        def call(handle, layout, row_elems, it=item, A=None, R=None):
            arrs = [pts(A or it[1]), pts(R or it[2][0]), F.ints_to_limbs([it[2][1]]), np.frombuffer(bytes(it[3]) + b"\0" * 8, dtype=np.uint8).copy()]
            out = np.full(1, 7, dtype=np.uint8)
            rc = lib.zk_eddsa_fill_hash_witnesses(handle, *[a.ctypes.data_as(C.c_void_p) for a in arrs], 1, C.c_void_p(buf.ptr), C.c_uint64(row_elems),
                                                  C.byref(J.EddsaHashLayout(*layout)), out.ctypes.data_as(C.c_void_p))
            assert rc == 0 or (out[0] == 7 and np.array_equal(buf.download(s.shape), s)), "a refused call wrote something"
            return rc

        far = 0xFFFFFF00
        assert call(mimc._h, lay, elems) == 1 and call(pure._h, lay, elems) == 1       # the scheme
        assert call(v._h, lay, elems - 1) == 1                                         # a short row
        assert call(v._h, lay3, lay3.n_vars + 1) == 1 and call(v3._h, lay, elems) == 1  # another msg_len
        assert call(v._h, lay._replace(msg_len=3), elems) == 1
        assert call(v._h, lay._replace(last_adder_var0=lay.last_adder_var0 + 1), elems) == 1        # leaves the row
        assert call(v._h, lay._replace(n_vars=lay.n_vars + 1), elems) == 1
        # the message hash at one byte: pad (1) | windows (3 x 2) | Montgomery adders (2 x 3) | converter (2) | no Edwards adder | bits | range | validator
        assert lay.m_edwards_adder_var0 == lay.m_bit0 and lay.m_window_var0 == lay.m_pad_bit0 + 1 and lay.m_pad_bit0 == lay.s_bit0 + 254
        for field, into in (("m_pad_bit0", -1), ("m_window_var0", -1), ("m_window_var0", 1), ("m_mont_adder_var0", -1), ("m_mont_adder_var0", 1),
                            ("m_converter_var0", -1), ("m_converter_var0", 1), ("m_bit0", -1), ("m_bit0", 1), ("m_range_var0", -1), ("m_range_var0", 1)):
            assert call(v._h, lay._replace(**{field: getattr(lay, field) + into}), elems) == 1, (field, into)       # into a neighbour
        for field in ("m_pad_bit0", "m_window_var0", "m_mont_adder_var0", "m_converter_var0", "m_bit0", "m_range_var0"):
            assert call(v._h, lay._replace(**{field: far}), elems) == 1, field                                      # out of the row
            assert call(v._h, lay._replace(**{field: 0}), elems) == 1, field                                        # variable 0 is ONE
        # 24 bytes: two segments, so the Edwards adder is there (7 variables between the converters and the bits) and no padding bit is
        assert lay24.m_bit0 - lay24.m_edwards_adder_var0 == 7 and lay24.m_window_var0 == lay24.m_pad_bit0
        for val in (lay24.m_edwards_adder_var0 - 1, lay24.m_edwards_adder_var0 + 1, far, 0):
            assert call(v24._h, lay24._replace(m_edwards_adder_var0=val), elems24, it=item24) == 1, val
        assert call(v._h, lay._replace(hash_window_var0=lay.ax_range_var0 + 98), elems) == 1        # the segments of the core are checked as before
        assert call(v._h, lay._replace(converter_var0=lay.converter_var0 - 1), elems) == 1
        assert call(v._h, lay._replace(step_stride=14), elems) == 1 and call(v._h, lay._replace(cond_var0=lay.doubler_var0 + 5), elems) == 1
        assert call(v._h, lay._replace(ax_var=0), elems) == 1
        assert call(v._h, lay, elems, A=(FR, 1)) == 1 and call(v._h, lay, elems, R=(0, FR)) == 1
        assert lib.zk_eddsa_fill_hash_witnesses(v._h, None, None, None, None, 1, None, C.c_uint64(elems), None, None) == 1
        assert lib.zk_eddsa_fill_hash_witnesses(v._h, None, None, None, None, 1, None, C.c_uint64(elems), C.byref(J.EddsaHashLayout(*lay)), None) == 1
        assert lib.zk_eddsa_fill_hash_witnesses(None, None, None, None, None, 0, None, C.c_uint64(elems), C.byref(J.EddsaHashLayout(*lay)), None) == 1
        assert np.array_equal(buf.download(s.shape), s)
        # an empty segment is empty, wherever its offset points: the same calls with nothing else wrong fill row 0
        assert call(v._h, lay._replace(m_edwards_adder_var0=0), elems) == 0 and call(v._h, lay._replace(m_edwards_adder_var0=far), elems) == 0
        assert call(v._h, lay._replace(m_edwards_adder_var0=lay.rx_var), elems) == 0 and call(v._h, lay, elems) == 0
        got = buf.download(s.shape)
        assert np.array_equal(got[0, :elems], F.fr_to_mont(HC.expected_row(v._hash_circuit, item))) and np.array_equal(got[0, elems:], s[0, elems:])
        assert np.array_equal(got[1], s[1])
        buf.upload(s)
        assert call(v24._h, lay24._replace(m_pad_bit0=0), elems24, it=item24) == 0 and call(v24._h, lay24._replace(m_pad_bit0=far), elems24, it=item24) == 0
        got = buf.download(s.shape)
        assert np.array_equal(got[0], F.fr_to_mont(HC.expected_row(v24._hash_circuit, item24))) and np.array_equal(got[1], s[1])
        assert v.fill_hash_witnesses([], [], [], buf)[0] == []                         # n = 0
        assert lib.zk_eddsa_fill_hash_witnesses(v._h, None, None, None, None, 0, None, C.c_uint64(elems), C.byref(J.EddsaHashLayout(*lay)), None) == 0
        assert np.array_equal(buf.download(s.shape), got)
        mitem = JC.signature_cases("mimc", 1)[0]
        for fn in (mimc.hash_circuit, pure.hash_circuit, lambda: mimc.fill_hash_witnesses([mitem[1]], [mitem[2]], [mitem[3]], buf),
                   lambda: pure.fill_hash_witnesses([item[1]], [item[2]], [item[3]], buf),
                   v.circuit, v.pedersen_circuit, lambda: v.fill_pedersen_witnesses([item[1]], [item[2]], [item[3]], buf)):
            try:
                fn()
                raise AssertionError("a scheme without this circuit was accepted")
            except NotImplementedError:
                pass
        for fn in (lambda: v24.fill_hash_witnesses([item24[1]] * 3, [item24[2]] * 3, [item24[3]] * 3, buf),   # a buffer of two rows
                   lambda: v.fill_hash_witnesses([item[1]], [item[2]], [b"ab"], buf),                         # two bytes for msg_len 1
                   lambda: v.fill_hash_witnesses([item[1]] * 2, [item[2]], [item[3]], buf)):                  # two keys, one signature
            try:
                fn()
                raise AssertionError("a call that cannot be right was accepted")
            except ValueError:
                pass
        buf.free()


def signed_items(J, msg_len=1):
    """three items from EdDSASigner("hash"): a valid signature, the same with the last message bit flipped, and s + L.  The expected verdicts are
    jubjub_cases.verify's"""
    msgs = [bytes([0x5A + i] * msg_len) for i in range(2)]
    with J.EdDSASigner("hash", msg_len=msg_len) as signer:
        A, sigs = signer.sign([0x1234567 + 2 * JC.L // 3, 0x7654321 + JC.L // 5], msgs)
    items = [("valid", A[0], sigs[0], msgs[0]), ("last bit of the message", A[0], sigs[0], JC.flip_last("hash", msgs[0])),
             ("s + L", A[1], (sigs[1][0], sigs[1][1] + JC.L), msgs[1])]
    items = [c + (JC.verify("hash", c[1], c[2], c[3]),) for c in items]
    assert [c[4] for c in items] == [True, False, True] and all(c[2][1] < HC.TWO254 for c in items)
    return items


def check_proofs(zk, J, items, accept, seed=47):
    """keygen on the circuit, the rows filled on the device, submit_batch(device_ptr=...).  The prover refuses a batch that holds the row of a
    wrong signature (ZK_ERR_DEGREE = 7) and goes on working; the items whose verdict is 1 are then filled side by side into a second buffer and
    proven in ONE submit of that many rows.  Returns the key and one proof text per item under the item's OWN public inputs: for a refused item
    the text of an accepted item's proof with the refused item's inputs, which is all a holder of a wrong signature can present"""
    k = len(items)
    with J.EdDSAVerifier("hash", msg_len=len(items[0][3])) as v:
        r, lay = v.hash_circuit()
        pk, vk = zk.keygen(r, seed=seed)
        verdicts, buf = v.fill_hash_witnesses([c[1] for c in items], [c[2] for c in items], [c[3] for c in items])
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
            again, rows = v.fill_hash_witnesses([items[p][1] for p in good], [items[p][2] for p in good], [items[p][3] for p in good])
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
            assert [int(x, 16) for x in json.loads(texts[p])["input"]] == v._hash_circuit.public_inputs(item[1], item[3])
        ctx.close(); buf.free()
    return vk, texts
