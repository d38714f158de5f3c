"""Baby JubJub on the device: the curve, the windowed Pedersen hash, batch EdDSA verification and batch EdDSA signing (zk_jj_*, zk_pedersen_*,
zk_eddsa_* of include/zkhip.h; kernels in csrc/jubjub.hpp and csrc/eddsa_sign.hpp).

The native surface of the reference's ethsnarks/jubjub.py, pedersen.py and eddsa.py, in bulk form: a point is a pair (x, y) of ints in [0, r),
the identity is (0, 1).  All curve arithmetic of a call runs in one HIP kernel launch; there is no CPU path.  A point that is not on
the curve raises ZkError (ZK_ERR_ARG) in scalar_mul / point_add / point_double / point_neg and as a base point, and gives the verdict False as
the A or R of a signature -- the reference never checks and divides by zero there; everything on the curve behaves as the reference does.

EdDSAVerifier("mimc").circuit() is the R1CS that proves such a signature (jubjub_gadgets.eddsa_mimc_circuit) and fill_witnesses writes the
complete witness rows of a batch into the device buffer that ProverContext.submit_batch(device_ptr=...) proves from.
EdDSAVerifier("pure").pedersen_circuit() and fill_pedersen_witnesses are the same pair for the reference's PureEdDSA gadget, whose hash is the
windowed Pedersen hash in the circuit (jubjub_gadgets.eddsa_pure_circuit, k_eddsa_fill_pure).
EdDSAVerifier("hash").hash_circuit() and fill_hash_witnesses are the pair for the reference's EdDSA gadget, which hashes the message in the
circuit first (jubjub_gadgets.EddsaHashCircuit, k_eddsa_fill_hash).

EdDSASigner is the reference's _SignatureScheme.sign in bulk: sign(keys, msgs) gives (A, sigs) in the shape verify() and the three fills take, so
sign -> verify -> fill witnesses -> prove runs on the device from end to end.  The kernel is not constant-time (include/zkhip.h): it is for bulk
generation of signatures, not for keys that must withstand a co-tenant of the device.
"""
import ctypes as C

import numpy as np

from . import fields as F
from . import jubjub_gadgets as JG
from . import prover as P

JUBJUB_Q = F.FR
JUBJUB_E = 21888242871839275222246405745257275088614511777268538073601725287587578984328
JUBJUB_C = 8
JUBJUB_L = JUBJUB_E // JUBJUB_C
JUBJUB_A = 168700
JUBJUB_D = 168696
SEGMENT_WINDOWS = 62
IDENTITY = (0, 1)
SCHEMES = {"mimc": 0, "pure": 1, "hash": 2}                     # ZK_EDDSA_*
_OPS = {"add": 0, "double": 1, "negate": 2}                     # ZK_JJ_OP_*
_SYMBOLS = ("zk_jj_hash_to_point", "zk_jj_pedersen_basepoint", "zk_jj_point_op", "zk_jj_scalar_mul", "zk_pedersen_create", "zk_pedersen_free",
            "zk_pedersen_hash", "zk_pedersen_table", "zk_eddsa_create", "zk_eddsa_free", "zk_eddsa_verify_batch", "zk_eddsa_fill_witnesses",
            "zk_eddsa_fill_pure_witnesses")
_HASH_FILL_SYMBOLS = ("zk_eddsa_fill_hash_witnesses",)           # checked by the first fill_hash_witnesses alone, likewise
_WIDE_FILL_SYMBOLS = ("zk_eddsa_fill_witnesses_wide",)           # checked by the first fill_witnesses(lanes > 1) alone, likewise
_SIGN_SYMBOLS = ("zk_eddsa_sign_batch", "zk_eddsa_sign_probe")   # checked by the signer alone: a library without them still serves the rest


class EddsaLayout(C.Structure):
    """zk_eddsa_layout: where the segments of a witness row of the MiMC-EdDSA circuit start (jubjub_gadgets.EddsaLayout, field for field)"""
    _fields_ = [(n, C.c_uint32) for n in JG.LAYOUT_FIELDS]


class EddsaPureLayout(C.Structure):
    """zk_eddsa_pure_layout: the segments of a witness row of the PureEdDSA circuit (jubjub_gadgets.EddsaPureLayout, field for field)"""
    _fields_ = [(n, C.c_uint32) for n in JG.PURE_LAYOUT_FIELDS]


class EddsaHashLayout(C.Structure):
    """zk_eddsa_hash_layout: the segments of a witness row of the EdDSA ("hash") circuit (jubjub_gadgets.EddsaHashLayout, field for field)"""
    _fields_ = [(n, C.c_uint32) for n in JG.HASH_LAYOUT_FIELDS]


def generator():
    """Point.generator() of the reference"""
    return (16540640123574156134436876038791482806971768689494387082833631921987005038935,
            20819045374670962167435360035096875258406992893633759881276124905556507972311)


def _lib():
    lib = P.load_library(P._lib_path_loaded)
    missing = [n for n in _SYMBOLS if not hasattr(lib, n)]
    if missing:
        raise ImportError("%s has no Baby JubJub entry points (%s ...): it was built without csrc/jubjub.cpp" % (P._lib_path_loaded or P.LIB_PATH, missing[0]))
    lib.zk_jj_hash_to_point.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    lib.zk_jj_pedersen_basepoint.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    lib.zk_pedersen_create.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.zk_pedersen_free.argtypes = [C.c_void_p]
    lib.zk_pedersen_free.restype = None
    lib.zk_pedersen_hash.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.zk_pedersen_table.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.zk_eddsa_create.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.zk_eddsa_free.argtypes = [C.c_void_p]
    lib.zk_eddsa_free.restype = None
    lib.zk_eddsa_verify_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    lib.zk_eddsa_fill_witnesses.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.zk_eddsa_fill_pure_witnesses.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def _hash_fill_lib():
    lib = _lib()
    missing = [n for n in _HASH_FILL_SYMBOLS if not hasattr(lib, n)]
    if missing:
        raise ImportError("%s has no witness fill for the EdDSA (\"hash\") circuit (%s): it was built before k_eddsa_fill_hash" % (P._lib_path_loaded or P.LIB_PATH, missing[0]))
    lib.zk_eddsa_fill_hash_witnesses.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def _wide_fill_lib():
    lib = _lib()
    missing = [n for n in _WIDE_FILL_SYMBOLS if not hasattr(lib, n)]
    if missing:
        raise ImportError("%s has no witness fill with several lanes per signature (%s): it was built before k_eddsa_fill_wide" % (P._lib_path_loaded or P.LIB_PATH, missing[0]))
    lib.zk_eddsa_fill_witnesses_wide.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


def _name(name):
    return name.encode("ascii") if isinstance(name, str) else bytes(name)


def _point_limbs(points):
    """[(x, y), ..] -> (n, 8) limbs; values of 256 bits pass (the library answers a coordinate >= r)"""
    flat = [int(c) for p in points for c in p]
    return F.ints_to_limbs(flat).reshape(-1, 8) if flat else np.zeros((0, 8), dtype=np.uint64)


def _points(arr):
    v = F.limbs_to_ints(arr)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def hash_to_point(data):
    """Point.from_hash(data)"""
    out = np.zeros(8, dtype=np.uint64)
    data = bytes(data)
    P._check(_lib().zk_jj_hash_to_point(data, len(data), _ptr(out)))
    return _points(out)[0]


def pedersen_basepoint(name, i):
    """pedersen_hash_basepoint(name, i) as an affine point"""
    out = np.zeros(8, dtype=np.uint64)
    P._check(_lib().zk_jj_pedersen_basepoint(_name(name), int(i), _ptr(out)))
    return _points(out)[0]


def _point_op(op, p, q, device):
    a = _point_limbs(p)
    b = _point_limbs(q) if q is not None else a
    if len(a) != len(b):
        raise ValueError("the point lists differ in length")
    out = np.zeros_like(a)
    if len(a):
        P._check(_lib().zk_jj_point_op(_OPS[op], P._p64(a), P._p64(b), C.c_uint32(len(a)), int(device), P._p64(out)))
    return _points(out)


def point_add(p, q, device=0):
    """[p_i + q_i] through the unified addition (also where p_i == q_i)"""
    return _point_op("add", p, q, device)


def point_double(p, device=0):
    """[2 p_i] through the dedicated doubling"""
    return _point_op("double", p, None, device)


def point_neg(p, device=0):
    return _point_op("negate", p, None, device)


def scalar_mul(points, scalars, device=0):
    """[k_i P_i]; k_i any integer in [0, 2^256)"""
    a = _point_limbs(points)
    ks = [int(k) for k in scalars]
    if len(ks) != len(a):
        raise ValueError("points and scalars differ in length")
    if any(not 0 <= k < 1 << 256 for k in ks):
        raise ValueError("a scalar is not in [0, 2^256)")
    out = np.zeros_like(a)
    if ks:
        k = F.ints_to_limbs(ks)
        P._check(_lib().zk_jj_scalar_mul(P._p64(a), P._p64(k), C.c_uint32(len(ks)), int(device), P._p64(out)))
    return _points(out)


def bits_to_windows(bits):
    """pedersen_hash_bits: 3-bit windows, the first bit the least significant; a last window of 1 or 2 bits is zero-padded"""
    bits = [int(b) for b in bits]
    return [sum(b << k for k, b in enumerate(bits[i:i + 3])) for i in range(0, len(bits), 3)]


def bytes_to_bits(data):
    """most significant bit first within each byte"""
    return [(byte >> (7 - k)) & 1 for byte in bytes(data) for k in range(8)]


def scalars_to_windows(scalars):
    """pedersen_hash_scalars: per scalar the windows (s >> i) & 7 for i in range(0, s.bit_length(), 3)"""
    return [(int(s) >> i) & 7 for s in scalars for i in range(0, int(s).bit_length(), 3)]


class PedersenHasher:
    """pedersen_hash_windows(name, ..) for inputs of up to max_bits bits (ceil(max_bits / 3) windows); the table of base-point multiples lives in
    device memory for the life of the object"""

    def __init__(self, name, max_bits, device=0):
        self._lib = _lib()
        self.name = _name(name)
        self.max_windows = (int(max_bits) + 2) // 3
        self._h = C.c_void_p()
        P._check(self._lib.zk_pedersen_create(self.name, self.max_windows, int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.zk_pedersen_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def hash_windows(self, rows):
        """[pedersen_hash_windows(name, row) for row in rows]; the rows may differ in length"""
        rows = [[int(w) for w in r] for r in rows]
        if not rows:
            return []
        stride = max(1, max(len(r) for r in rows))
        win = np.zeros((len(rows), stride), dtype=np.uint8)
        for i, r in enumerate(rows):
            if any(not 0 <= w < 256 for w in r):
                raise ValueError("a window is not a byte")
            win[i, :len(r)] = r
        counts = np.array([len(r) for r in rows], dtype=np.uint32)
        out = np.zeros((len(rows), 8), dtype=np.uint64)
        P._check(self._lib.zk_pedersen_hash(self._h, _ptr(win), _ptr(counts), stride, len(rows), _ptr(out)))
        return _points(out)

    def hash_bits(self, rows):
        """[pedersen_hash_bits(name, bits) for bits in rows]; bits: a sequence of 0 / 1 or a str of them"""
        return self.hash_windows([bits_to_windows(r) for r in rows])

    def hash_bytes(self, rows):
        """[pedersen_hash_bytes(name, data) for data in rows]"""
        return self.hash_windows([bits_to_windows(bytes_to_bits(r)) for r in rows])

    def hash_scalars(self, rows):
        """[pedersen_hash_scalars(name, *row) for row in rows]; a row without windows (all scalars 0) hashes to the identity, as in the reference"""
        wins = [scalars_to_windows(r) for r in rows]
        full = [i for i, w in enumerate(wins) if w]
        got = dict(zip(full, self.hash_windows([wins[i] for i in full])))
        return [got.get(i, IDENTITY) for i in range(len(wins))]

    def table(self, first_window, n_windows):
        """the table points [(1 .. 4) 16^(j % 62) B_(j / 62)] of n_windows window positions from first_window on"""
        out = np.zeros((int(n_windows) * 4, 8), dtype=np.uint64)
        P._check(self._lib.zk_pedersen_table(self._h, int(first_window), int(n_windows), _ptr(out)))
        pts = _points(out)
        return [pts[4 * i:4 * i + 4] for i in range(int(n_windows))]


class EdDSAVerifier:
    """Batch verification of one scheme: "mimc" (MiMCEdDSA; a message is msg_len field elements), "pure" (PureEdDSA; msg_len bytes) or "hash"
    (EdDSA; msg_len bytes).  B=None: the generator.  verify gives the reference's verdict S B == R + H(R, A, M) A for every item"""

    def __init__(self, scheme, B=None, msg_len=1, device=0):
        self._lib = _lib()
        self.scheme = scheme
        self.msg_len = int(msg_len)
        self.B = (int(B[0]), int(B[1])) if B is not None else None
        self._circuit = None
        self._pedersen_circuit = None
        self._hash_circuit = None
        self._h = C.c_void_p()
        b = _point_limbs([B]) if B is not None else None
        P._check(self._lib.zk_eddsa_create(SCHEMES[scheme], _ptr(b) if b is not None else None, self.msg_len, int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.zk_eddsa_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _items(self, A, sigs, msgs):
        sigs = list(sigs)
        n = len(sigs)
        A = list(A)
        if len(A) == 2 and not isinstance(A[0], (tuple, list)):
            A = [tuple(A)] * n
        msgs = list(msgs)
        if len(A) != n or len(msgs) != n:
            raise ValueError("A, sigs and msgs differ in length")
        return A, sigs, msgs, n

    def _circuit_object(self):
        if self.scheme != "mimc":
            raise NotImplementedError('only the "mimc" scheme has the MiMC circuit; "%s" has %s' % (
                self.scheme, "pedersen_circuit() and fill_pedersen_witnesses" if self.scheme == "pure" else "hash_circuit() and fill_hash_witnesses"))
        if self._circuit is None:
            self._circuit = JG.EddsaMimcCircuit(self.msg_len, self.B)
        return self._circuit

    def circuit(self):
        """(R1CS, layout) of the circuit that accepts this verifier's signatures: jubjub_gadgets.eddsa_mimc_circuit for its msg_len and B.  Public
        inputs: A.x, A.y, the message elements.  layout: a jubjub_gadgets.EddsaLayout; a witness row has layout.n_vars + 1 elements"""
        c = self._circuit_object()
        return c.r1cs(), c.layout

    def fill_witnesses(self, A, sigs, msgs, out=None, row_elems=None, layout=None, lanes=1):
        """The complete witness rows of the circuit for a batch, written on the device, Montgomery, ready for submit_batch(device_ptr=...):
        row i of `out` (a prover.DeviceBuffer or a device address; None: a new DeviceBuffer) belongs to signature i.  Returns (verdicts, out).
        A wrong signature still gets its row (only the two closing constraints fail; the prover refuses a batch that holds it: ZK_ERR_DEGREE); an item with A or R off the curve or s >= 2^254 gets the
        verdict False and its row is left as it was.  s may be any integer below 2^256.  A, sigs, msgs as verify().
        lanes: 1 (one lane walks a signature's whole row), 2 or 4 (that many lanes share it: zk_eddsa_fill_witnesses_wide -- the same rows, a shorter
        dependent chain, for small batches).  The caller chooses; nothing here does"""
        if lanes not in (1, 2, 4):
            raise ValueError("lanes per signature: 1, 2 or 4")
        wide = _wide_fill_lib() if lanes != 1 else None
        c = self._circuit_object()
        if wide is None:
            return self._fill(self._lib.zk_eddsa_fill_witnesses, EddsaLayout, c.layout, A, sigs, msgs, out=out, row_elems=row_elems, layout=layout)
        return self._fill(wide.zk_eddsa_fill_witnesses_wide, EddsaLayout, c.layout, A, sigs, msgs, out=out, row_elems=row_elems, layout=layout, extra=(lanes,))

    def _fill(self, entry, layout_type, circuit_layout, A, sigs, msgs, *, out, row_elems, layout, byte_msgs=False, extra=()):
        """What fill_witnesses, fill_pedersen_witnesses and fill_hash_witnesses share: checks the batch, packs it and calls `entry`, the library's
        fill of one circuit, with the row layout as a `layout_type` and `extra` behind its arguments.  byte_msgs: a message is msg_len bytes, not msg_len field elements"""
        A, sigs, msgs, n = self._items(A, sigs, msgs)
        lay = circuit_layout if layout is None else layout
        if row_elems is None:
            row_elems = lay.n_vars + 1
        if byte_msgs:
            msgs = [bytes(m) for m in msgs]
        if any(len(m) != self.msg_len for m in msgs):
            raise ValueError("a message does not have msg_len %s" % ("bytes" if byte_msgs else "elements"))
        if out is None:
            out = P.DeviceBuffer(32 * int(row_elems) * max(n, 1))
        if isinstance(out, P.DeviceBuffer) and n * int(row_elems) * 32 > out.nbytes:
            raise ValueError("the device buffer is smaller than n rows")
        ptr = out.ptr if isinstance(out, P.DeviceBuffer) else int(out)
        a = _point_limbs(A)
        r = _point_limbs([R for R, _ in sigs])
        s = F.ints_to_limbs([int(v) for _, v in sigs]) if n else np.zeros((0, 4), dtype=np.uint64)
        if byte_msgs:
            m = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
        else:
            m = F.ints_to_limbs([int(v) for msg in msgs for v in msg]) if n else np.zeros((0, 4), dtype=np.uint64)
        verdicts = np.full(max(n, 1), 255, dtype=np.uint8)
        P._check(entry(self._h, _ptr(a), _ptr(r), _ptr(s), _ptr(m), n, C.c_void_p(ptr), C.c_uint64(int(row_elems)), C.byref(layout_type(*lay)),
                       _ptr(verdicts), *extra))
        return [bool(v) for v in verdicts[:n]], out

    def _pedersen_circuit_object(self):
        if self.scheme != "pure":
            raise NotImplementedError('only the "pure" scheme has the PureEdDSA circuit; "mimc" has circuit() and fill_witnesses, "hash" has '
                                      'hash_circuit() and fill_hash_witnesses')
        if self._pedersen_circuit is None:
            self._pedersen_circuit = JG.EddsaPureCircuit(self.msg_len, self.B)
        return self._pedersen_circuit

    def pedersen_circuit(self):
        """(R1CS, layout) of the PureEdDSA circuit that accepts this verifier's signatures: jubjub_gadgets.eddsa_pure_circuit for its msg_len and
        B.  Public inputs: A.x, A.y, the 8 msg_len message bits.  layout: a jubjub_gadgets.EddsaPureLayout; a row has layout.n_vars + 1 elements.
        (circuit() keeps its meaning: the MiMC circuit, which only "mimc" has)"""
        c = self._pedersen_circuit_object()
        return c.r1cs(), c.layout

    def fill_pedersen_witnesses(self, A, sigs, msgs, out=None, row_elems=None, layout=None):
        """fill_witnesses for the PureEdDSA circuit: the complete rows of a batch written on the device, Montgomery, ready for
        submit_batch(device_ptr=...).  Returns (verdicts, out).  A wrong signature still gets its row; an item with A or R off the curve or
        s >= 2^254 gets the verdict False and its row is left as it was.  A, sigs, msgs as verify(); the circuit, unlike verify(), refuses an R of
        low order and takes any s below 2^254"""
        c = self._pedersen_circuit_object()
        return self._fill(self._lib.zk_eddsa_fill_pure_witnesses, EddsaPureLayout, c.layout, A, sigs, msgs, out=out, row_elems=row_elems, layout=layout,
                          byte_msgs=True)

    def _hash_circuit_object(self):
        if self.scheme != "hash":
            raise NotImplementedError('only the "hash" scheme has the EdDSA circuit that hashes the message first; "mimc" has circuit() and '
                                      'fill_witnesses, "pure" has pedersen_circuit() and fill_pedersen_witnesses')
        if self._hash_circuit is None:
            self._hash_circuit = JG.EddsaHashCircuit(self.msg_len, self.B)
        return self._hash_circuit

    def hash_circuit(self):
        """(R1CS, layout) of the EdDSA circuit that accepts this verifier's signatures: jubjub_gadgets.EddsaHashCircuit for its msg_len and B, the
        message hashed in the circuit ("EdDSA_Verify.M") before PureEdDSA over the bits of that hash.  Public inputs: A.x, A.y, the 8 msg_len
        message bits.  layout: a jubjub_gadgets.EddsaHashLayout; a row has layout.n_vars + 1 elements"""
        c = self._hash_circuit_object()
        return c.r1cs(), c.layout

    def fill_hash_witnesses(self, A, sigs, msgs, out=None, row_elems=None, layout=None):
        """fill_pedersen_witnesses for the circuit of hash_circuit(): the complete rows of a batch written on the device, Montgomery, ready for
        submit_batch(device_ptr=...).  Returns (verdicts, out).  A wrong signature still gets its row; an item with A or R off the curve or
        s >= 2^254 gets the verdict False and its row is left as it was.  A, sigs, msgs as verify(); the circuit, unlike verify(), refuses an R of
        low order and takes any s below 2^254.  ImportError from a library that was built before this entry point"""
        c = self._hash_circuit_object()
        lib = _hash_fill_lib()
        return self._fill(lib.zk_eddsa_fill_hash_witnesses, EddsaHashLayout, c.layout, A, sigs, msgs, out=out, row_elems=row_elems, layout=layout,
                          byte_msgs=True)

    def verify(self, A, sigs, msgs):
        """A: one public key per signature (or a single point for all); sigs: [(R, s), ..]; msgs: bytes objects (lists of ints for "mimc")"""
        sigs = list(sigs)
        if len(sigs) == 0:
            return []
        A, sigs, msgs, n = self._items(A, sigs, msgs)
        a = _point_limbs(A)
        r = _point_limbs([R for R, _ in sigs])
        s = F.ints_to_limbs([int(v) for _, v in sigs])
        if self.scheme == "mimc":
            if any(len(m) != self.msg_len for m in msgs):
                raise ValueError("a message does not have msg_len elements")
            m = F.ints_to_limbs([int(v) for msg in msgs for v in msg])
        else:
            if any(len(bytes(m)) != self.msg_len for m in msgs):
                raise ValueError("a message does not have msg_len bytes")
            m = np.frombuffer(b"".join(bytes(x) for x in msgs), dtype=np.uint8).copy()
        out = np.full(n, 255, dtype=np.uint8)
        P._check(self._lib.zk_eddsa_verify_batch(self._h, _ptr(a), _ptr(r), _ptr(s), _ptr(m), n, _ptr(out)))
        return [bool(v) for v in out]


def _sign_lib():
    lib = _lib()
    missing = [n for n in _SIGN_SYMBOLS if not hasattr(lib, n)]
    if missing:
        raise ImportError("%s has no EdDSA signer (%s): it was built before csrc/eddsa_sign.hpp" % (P._lib_path_loaded or P.LIB_PATH, missing[0]))
    lib.zk_eddsa_sign_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 3
    lib.zk_eddsa_sign_probe.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    return lib


class EdDSASigner:
    """Batch signing of one scheme -- _SignatureScheme.sign of the reference for "mimc" (a message is msg_len field elements), "pure" or "hash"
    (msg_len bytes).  B=None: the generator.  Owns a zk_eddsa handle like EdDSAVerifier; the first sign() builds the fixed-base table of B on it.
    Deterministic: r = SHA-512(key || M) mod L.  Not constant-time (include/zkhip.h)"""

    def __init__(self, scheme, B=None, msg_len=1, device=0):
        self._h = C.c_void_p()                                  # (first: close() runs from __del__ even when the line below raises)
        self._lib = _sign_lib()
        self.scheme = scheme
        self.msg_len = int(msg_len)
        self.B = (int(B[0]), int(B[1])) if B is not None else None
        b = _point_limbs([B]) if B is not None else None
        P._check(self._lib.zk_eddsa_create(SCHEMES[scheme], _ptr(b) if b is not None else None, self.msg_len, int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.zk_eddsa_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sign(self, keys, msgs):
        """keys: ints in (0, L); msgs: bytes objects (lists of ints for "mimc"), one per key.  Returns (A, sigs): the public keys key B as points
        and [(R, s), ..], what EdDSAVerifier.verify(A, sigs, msgs) and the three fills take.  s is the integer mod 8 L.
        ZkError (ZK_ERR_ARG) for a key that is 0 or >= L or a "mimc" message element >= r; nothing is signed then"""
        keys = [int(k) for k in keys]
        msgs = list(msgs)
        n = len(keys)
        if len(msgs) != n:
            raise ValueError("keys and msgs differ in length")
        if n == 0:
            return [], []
        if any(not 0 <= k < 1 << 256 for k in keys):
            raise ValueError("a key is not in [0, 2^256)")
        if self.scheme == "mimc":
            if any(len(m) != self.msg_len for m in msgs):
                raise ValueError("a message does not have msg_len elements")
            m = F.ints_to_limbs([int(x) for msg in msgs for x in msg])
        else:
            if any(len(bytes(m)) != self.msg_len for m in msgs):
                raise ValueError("a message does not have msg_len bytes")
            m = np.frombuffer(b"".join(bytes(x) for x in msgs), dtype=np.uint8).copy()
        k = F.ints_to_limbs(keys)
        a = np.zeros((n, 8), dtype=np.uint64)
        r = np.zeros((n, 8), dtype=np.uint64)
        s = np.zeros((n, 4), dtype=np.uint64)
        try:
            P._check(self._lib.zk_eddsa_sign_batch(self._h, _ptr(k), _ptr(m), n, _ptr(a), _ptr(r), _ptr(s)))
        finally:
            k.fill(0)                                           # the staging copy of the keys
        return _points(a), list(zip(_points(r), F.limbs_to_ints(s)))
