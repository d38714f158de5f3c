"""Merkle trees in device memory: MiMC (node width 2) and Poseidon (node width 2, 3 or 4) (zk_mtree_* of include/zkhip.h; kernels in csrc/merkle.hpp).

The surface of the reference's ethsnarks/merkletree.py (MerkleTree over MerkleHasher_MiMC, width 2): append, update, proof, root,
leaf(depth, offset) -- plus the bulk forms a GPU needs: extend, update_many, proofs, and fill_witnesses, which writes the inputs of the
membership circuit (gadgets.merkle_membership_circuit) for k leaves straight into a device witness buffer, ready for
prover.WitnessPlan.solve and ProverContext.submit_batch(device_ptr=...).  fill_full_witnesses writes the COMPLETE witness instead -- every node
of a path is in the tree, so one lane per (row, level) computes the level's selector and hash variables and nothing is left for the planner:
tree -> fill_full_witnesses -> submit_batch(device_ptr=...).  update_seq applies k leaf updates IN ORDER (an index may repeat) and writes per update
the complete witness of the root-to-root transition circuit (gadgets.merkle_update_circuit): tree -> update_seq -> submit_batch(device_ptr=...).
All hashing runs in HIP kernels; there is no CPU path.

MerkleTree(n, hasher="poseidon", width=w) is the reference's MerkleTree over MerkleHasher_Poseidon (csrc/poseidon.hpp): n = w^depth leaf slots,
proofs with w - 1 siblings per level; poseidon_hash / poseidon_permute / poseidon_constants expose the permutation itself.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import fields as F
from . import gadgets as G
from . import prover as P

MAX_DEPTH = 29
_SYMBOLS = ("zk_mtree_create", "zk_mtree_free", "zk_mtree_size", "zk_mtree_append", "zk_mtree_append_resident", "zk_mtree_update",
            "zk_mtree_root", "zk_mtree_node", "zk_mtree_paths", "zk_mtree_fill_witnesses", "zk_mimc_constants", "zk_mimc_hash2",
            "zk_mtree_create_ex", "zk_mtree_info", "zk_poseidon_constants", "zk_poseidon_hash", "zk_poseidon_permute",
            "zk_mtree_fill_full_witnesses", "zk_mtree_update_seq")
HASHERS = {"mimc": 0, "poseidon": 1}                          # ZK_MTREE_HASH_*


class Layout(C.Structure):
    """zk_mtree_layout: the variable indices of the membership circuit's inputs in a witness row"""
    _fields_ = [(n, C.c_uint32) for n in ("root_var", "addr_var0", "path_var0", "leaf_var", "iv_var0", "n_iv")]


def membership_layout(depth, hasher="mimc"):
    """the allocation order of merkle_membership_circuit / merkle_path_authenticator: root, address bits, path, leaf, 29 IVs;
    poseidon_membership_circuit has the same order and no IVs"""
    if hasher == "poseidon":
        return Layout(1, 2, 2 + depth, 2 + 2 * depth, 0, 0)
    return Layout(1, 2, 2 + depth, 2 + 2 * depth, 3 + 2 * depth, 29)


LEVEL_VARS = {"mimc": 736, "poseidon": 322}                  # selector + hash variables of one level (csrc/merkle.hpp)


def membership_full_layout(depth, hasher="mimc"):
    """(Layout, level_var0, level_stride, row_elems) of the complete witness of merkle_membership_circuit / poseidon_membership_circuit: the
    inputs of membership_layout, then per level the six selector variables and the hash gadget's variables, in allocation order"""
    layout = membership_layout(depth, hasher)
    level_var0 = 3 + 2 * depth + layout.n_iv
    stride = LEVEL_VARS[hasher]
    return layout, level_var0, stride, level_var0 + stride * depth


class UpdateLayout(C.Structure):
    """zk_mtree_update_layout: the variable indices of the update circuit's inputs in a witness row"""
    _fields_ = [(n, C.c_uint32) for n in ("old_root_var", "new_root_var", "addr_var0", "path_var0", "old_leaf_var", "new_leaf_var", "iv_var0", "n_iv")]


def update_layout(depth, hasher="mimc"):
    """(UpdateLayout, level_var0, level_stride, row_elems) of the complete witness of gadgets.merkle_update_circuit: old_root, new_root, address
    bits, path, old_leaf, new_leaf, (29 IVs,) then the level blocks of the old chain and those of the new chain"""
    n_iv = 0 if hasher == "poseidon" else 29
    layout = UpdateLayout(1, 2, 3, 3 + depth, 3 + 2 * depth, 4 + 2 * depth, 5 + 2 * depth if n_iv else 0, n_iv)
    level_var0 = 5 + 2 * depth + n_iv
    stride = LEVEL_VARS[hasher]
    return layout, level_var0, stride, level_var0 + 2 * stride * depth


def _lib():
    """the loaded library, checked for the tree's entry points (the CPU emulation of the prover alone does not have them)"""
    lib = P.load_library(P._lib_path_loaded)
    missing = [n for n in _SYMBOLS if not hasattr(lib, n)]
    if missing:
        raise ImportError("%s has no Merkle tree entry points (%s ...): it was built without csrc/merkle.cpp" % (P._lib_path_loaded or P.LIB_PATH, missing[0]))
    return lib


def _leaf_limbs(values):
    """ints in [0, r) -> canonical (n, 4) limbs; a numpy (n, 4) uint64 array is taken as canonical limbs as it is"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint64 and values.ndim == 2 and values.shape[1] == 4:
        return np.ascontiguousarray(values)
    vals = [int(v) for v in values]
    for v in vals:
        if not 0 <= v < F.FR:
            raise ValueError("leaf %d is not in [0, r)" % v)
    return F.ints_to_limbs(vals) if vals else np.zeros((0, 4), dtype=np.uint64)


def mimc_constants():
    """(round constants, level IVs) as the kernels use them"""
    rc = np.zeros((91, 4), dtype=np.uint64)
    iv = np.zeros((MAX_DEPTH, 4), dtype=np.uint64)
    P._check(_lib().zk_mimc_constants(P._p64(rc), P._p64(iv)))
    return F.limbs_to_ints(rc), F.limbs_to_ints(iv)


def mimc_hash2(left, right, iv, device=0):
    """[mimc_hash([l, r], iv) for l, r, iv in zip(left, right, iv)] on the device"""
    a, b, c = (F.ints_to_limbs([int(v) for v in x]) for x in (left, right, iv))
    if not (len(a) == len(b) == len(c)):
        raise ValueError("left, right and iv differ in length")
    out = np.zeros_like(a)
    if len(a):
        P._check(_lib().zk_mimc_hash2(P._p64(a), P._p64(b), P._p64(c), C.c_uint32(len(a)), int(device), P._p64(out)))
    return F.limbs_to_ints(out)


def poseidon_constants():
    """(C, M) as the kernels use them: 65 round constants, the 6 x 6 matrix as a list of rows"""
    c = np.zeros((65, 4), dtype=np.uint64)
    m = np.zeros((36, 4), dtype=np.uint64)
    P._check(_lib().zk_poseidon_constants(P._p64(c), P._p64(m)))
    mv = F.limbs_to_ints(m)
    return F.limbs_to_ints(c), [mv[6 * i:6 * i + 6] for i in range(6)]


def poseidon_hash(inputs, device=0):
    """[poseidon(row) for row in inputs] on the device; every row has the same length, 1 .. 5"""
    rows = [[int(v) for v in row] for row in inputs]
    if not rows:
        return []
    n_in = len(rows[0])
    if any(len(r) != n_in for r in rows):
        raise ValueError("the input lists differ in length")
    a = F.ints_to_limbs([v for r in rows for v in r]) if n_in else np.zeros((0, 4), dtype=np.uint64)
    out = np.zeros((len(rows), 4), dtype=np.uint64)
    P._check(_lib().zk_poseidon_hash(P._p64(a), C.c_uint32(n_in), C.c_uint32(len(rows)), int(device), P._p64(out)))
    return F.limbs_to_ints(out)


def poseidon_permute(states, device=0):
    """the chained form: every six-element state through the permutation, on the device"""
    rows = [[int(v) for v in row] for row in states]
    if not rows:
        return []
    if any(len(r) != 6 for r in rows):
        raise ValueError("a state has six elements")
    a = F.ints_to_limbs([v for r in rows for v in r])
    P._check(_lib().zk_poseidon_permute(P._p64(a), C.c_uint32(len(rows)), int(device)))
    v = F.limbs_to_ints(a)
    return [v[6 * i:6 * i + 6] for i in range(len(rows))]


class MerkleProof(namedtuple("MerkleProof", "leaf address path width hasher", defaults=(2, "mimc"))):
    """leaf, address digits (level 0 first; bits at width 2) and siblings of one leaf: one sibling per level at width 2, a list of
    width - 1 per level above that (the other children of the parent, in node order)"""

    def verify(self, root):
        if self.hasher == "mimc":
            return G.merkle_root(self.leaf, self.address, self.path, G.merkle_ivs(MAX_DEPTH)) == root
        item = self.leaf
        for digit, sibs in zip(self.address, self.path):
            args = list(sibs) if isinstance(sibs, list) else [sibs]
            args.insert(digit, item)
            item = G.poseidon(args)
        return item == root


class MerkleTree:
    """A tree of n_items = width^depth leaf slots resident on `device`: hasher "mimc" (width 2, depth 1 .. 29) or "poseidon" (width 2, 3, 4;
    at most 2^29 leaf slots)."""

    def __init__(self, n_items, device=0, reserve=0, *, width=2, hasher="mimc"):
        n_items, width = int(n_items), int(width)
        if hasher not in HASHERS:
            raise ValueError("hasher must be 'mimc' or 'poseidon'")
        if width < 2:
            raise ValueError("the node width must be at least 2")
        depth, cap = 0, 1
        while cap < n_items:
            cap *= width
            depth += 1
        if n_items < 2 or cap != n_items:
            raise ValueError("n_items must be a power of two >= 2" if width == 2 else "n_items must be a power of the width")
        self.n_items, self.depth, self.device, self.width, self.hasher = n_items, depth, int(device), width, hasher
        h = C.c_void_p()
        if hasher == "mimc" and width == 2:
            P._check(_lib().zk_mtree_create(C.c_uint32(depth), C.c_uint64(reserve), self.device, C.byref(h)))
        else:
            P._check(_lib().zk_mtree_create_ex(C.c_uint32(depth), C.c_uint32(width), HASHERS[hasher], C.c_uint64(reserve), self.device, C.byref(h)))
        self._h = h

    # ---- size
    def __len__(self):
        n = C.c_uint64(0)
        P._check(P._lib.zk_mtree_size(self._h, C.byref(n)))
        return int(n.value)

    # ---- writing
    def extend(self, leaves, n=None, canonical=True):
        """append many leaves: ints, canonical (n, 4) limbs, or a prover.DeviceBuffer holding n elements (Montgomery unless canonical)"""
        if isinstance(leaves, P.DeviceBuffer):
            if n is None:
                n = leaves.nbytes // 32
            P._check(P._lib.zk_mtree_append_resident(self._h, C.c_void_p(leaves.ptr), C.c_uint64(n), int(canonical)))
            return
        a = _leaf_limbs(leaves)
        if len(a):
            P._check(P._lib.zk_mtree_append(self._h, P._p64(a), C.c_uint64(len(a)), int(canonical)))

    def append(self, leaf):
        """returns the index of the new leaf"""
        i = len(self)
        self.extend([leaf])
        return i

    def update_many(self, indices, leaves):
        """leaves[j] replaces leaf indices[j]; the last occurrence of an index wins"""
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        a = _leaf_limbs(leaves)
        if len(idx) != len(a):
            raise ValueError("indices and leaves differ in length")
        if len(idx):
            P._check(P._lib.zk_mtree_update(self._h, P._p64(idx), P._p64(a), C.c_uint32(len(idx)), 1))

    def update(self, index, leaf):
        self.update_many([index], [leaf])

    def __setitem__(self, index, leaf):
        self.update(index, leaf)

    # ---- reading
    def leaf(self, depth, offset):
        """any node: level `depth` (0 = leaves), position `offset`; the placeholder where the tree holds nothing yet"""
        out = np.zeros(4, dtype=np.uint64)
        P._check(P._lib.zk_mtree_node(self._h, C.c_uint32(depth), C.c_uint64(offset), P._p64(out)))
        return F.limbs_to_ints(out)[0]

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError("leaf index out of range")
        return self.leaf(0, index)

    @property
    def root(self):
        if len(self) == 0:
            return None
        out = np.zeros(4, dtype=np.uint64)
        P._check(P._lib.zk_mtree_root(self._h, P._p64(out)))
        return F.limbs_to_ints(out)[0]

    def proofs(self, indices):
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        k = len(idx)
        if k == 0:
            return []
        leaves = np.zeros((k, 4), dtype=np.uint64)
        D, w = self.depth, self.width
        paths = np.zeros((k * D * (w - 1), 4), dtype=np.uint64)
        P._check(P._lib.zk_mtree_paths(self._h, P._p64(idx), C.c_uint32(k), P._p64(leaves), P._p64(paths)))
        lv, pv = F.limbs_to_ints(leaves), F.limbs_to_ints(paths)
        if w == 2:
            return [MerkleProof(lv[j], [(int(idx[j]) >> d) & 1 for d in range(D)], pv[j * D:(j + 1) * D], 2, self.hasher) for j in range(k)]
        out, S = [], D * (w - 1)
        for j in range(k):
            digits = [int(idx[j]) // w ** d % w for d in range(D)]
            out.append(MerkleProof(lv[j], digits, [pv[j * S + d * (w - 1):j * S + (d + 1) * (w - 1)] for d in range(D)], w, self.hasher))
        return out

    def proof(self, index):
        return self.proofs([index])[0]

    def fill_witnesses(self, indices, device_buffer, r1cs_or_layout=None, row_elems=None):
        """rows 0 .. k - 1 of a device witness buffer get ONE, the root, the address bits, the path, the leaf and the IVs of the given
        leaves (Montgomery).  r1cs_or_layout: the constraint system of merkle_membership_circuit(depth) (row = V + 1 elements, its
        allocation order), or a Layout together with row_elems.  device_buffer: a prover.DeviceBuffer or a device pointer."""
        if isinstance(r1cs_or_layout, Layout):
            layout = r1cs_or_layout
            if row_elems is None:
                raise ValueError("a Layout needs row_elems")
        else:
            layout = membership_layout(self.depth, self.hasher)
            if row_elems is None:
                if r1cs_or_layout is None:
                    raise ValueError("give the constraint system, or a Layout and row_elems")
                row_elems = r1cs_or_layout.V + 1
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        ptr = device_buffer.ptr if isinstance(device_buffer, P.DeviceBuffer) else int(device_buffer)
        if isinstance(device_buffer, P.DeviceBuffer) and len(idx) * int(row_elems) * 32 > device_buffer.nbytes:
            raise ValueError("the device buffer is smaller than k rows")
        if len(idx):
            P._check(P._lib.zk_mtree_fill_witnesses(self._h, P._p64(idx), C.c_uint32(len(idx)), C.c_void_p(ptr), C.c_uint64(row_elems), C.byref(layout)))

    def fill_full_witnesses(self, indices, device_buffer, r1cs_or_layout=None, row_elems=None, level_var0=None, level_stride=None):
        """rows 0 .. k - 1 of a device witness buffer get the COMPLETE witness of the membership circuit of the given leaves (Montgomery,
        canonical): what fill_witnesses writes, and every level's selector and hash variables, computed from the nodes of the tree -- byte for
        byte what WitnessPlan.solve would leave, ready for submit_batch(device_ptr=...).  Arguments as fill_witnesses; level_var0 and
        level_stride place the level blocks (default: the allocation order, membership_full_layout)."""
        _, var0, stride, _ = membership_full_layout(self.depth, self.hasher)
        if isinstance(r1cs_or_layout, Layout):
            layout = r1cs_or_layout
            if row_elems is None:
                raise ValueError("a Layout needs row_elems")
        else:
            layout = membership_layout(self.depth, self.hasher)
            if row_elems is None:
                if r1cs_or_layout is None:
                    raise ValueError("give the constraint system, or a Layout and row_elems")
                row_elems = r1cs_or_layout.V + 1
        level_var0 = var0 if level_var0 is None else int(level_var0)
        level_stride = stride if level_stride is None else int(level_stride)
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        ptr = device_buffer.ptr if isinstance(device_buffer, P.DeviceBuffer) else int(device_buffer)
        if isinstance(device_buffer, P.DeviceBuffer) and len(idx) * int(row_elems) * 32 > device_buffer.nbytes:
            raise ValueError("the device buffer is smaller than k rows")
        P._check(_lib().zk_mtree_fill_full_witnesses(self._h, P._p64(idx), C.c_uint32(len(idx)), C.c_void_p(ptr), C.c_uint64(row_elems), C.byref(layout),
                                                     C.c_uint32(level_var0), C.c_uint32(level_stride)))

    def update_seq(self, indices, leaves, device_buffer=None, r1cs_or_layout=None, row_elems=None, level_var0=None, level_stride=None):
        """leaves[j] replaces leaf indices[j], IN THE GIVEN ORDER: an index may repeat, and update j sees updates 0 .. j - 1.  Returns the k + 1
        roots [before, after update 0, .., after update k - 1] as ints; the tree ends up as after k single update() calls.  With a
        device_buffer (a prover.DeviceBuffer or a device pointer), row j receives the COMPLETE witness of gadgets.merkle_update_circuit for
        update j -- "replacing leaf a_j (old value x) by y takes root R_j to R_{j+1}", byte for byte what WitnessPlan.solve would leave --
        ready for submit_batch(device_ptr=...).  r1cs_or_layout: the constraint system of merkle_update_circuit(depth, hasher) (row = V + 1
        elements), or an UpdateLayout together with row_elems; level_var0 and level_stride place the level blocks (default: update_layout)."""
        lib = _lib()
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        a = _leaf_limbs(leaves)
        k = len(idx)
        if k != len(a):
            raise ValueError("indices and leaves differ in length")
        layout, var0, stride, _ = update_layout(self.depth, self.hasher)
        ptr = None
        if device_buffer is not None:
            if isinstance(r1cs_or_layout, UpdateLayout):
                layout = r1cs_or_layout
                if row_elems is None:
                    raise ValueError("an UpdateLayout needs row_elems")
            elif row_elems is None:
                if r1cs_or_layout is None:
                    raise ValueError("give the constraint system, or an UpdateLayout and row_elems")
                row_elems = r1cs_or_layout.V + 1
            ptr = device_buffer.ptr if isinstance(device_buffer, P.DeviceBuffer) else int(device_buffer)
            if isinstance(device_buffer, P.DeviceBuffer) and k * int(row_elems) * 32 > device_buffer.nbytes:
                raise ValueError("the device buffer is smaller than k rows")
        level_var0 = var0 if level_var0 is None else int(level_var0)
        level_stride = stride if level_stride is None else int(level_stride)
        roots = np.zeros((k + 1, 4), dtype=np.uint64)
        P._check(lib.zk_mtree_update_seq(self._h, P._p64(idx), P._p64(a), C.c_uint32(k), 1, C.c_void_p(ptr), C.c_uint64(row_elems or 0), C.byref(layout),
                                         C.c_uint32(level_var0), C.c_uint32(level_stride), P._p64(roots)))
        return F.limbs_to_ints(roots)

    def close(self):
        if getattr(self, "_h", None) is not None and P._lib is not None:
            P._lib.zk_mtree_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
