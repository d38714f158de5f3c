// merkle.hpp -- MiMC-e7 Miyaguchi-Preneel hashing and the kernels of the device Merkle tree (merkle.cpp, zk_mtree_* of include/zkhip.h).
//
// The tree of ethsnarks/merkletree.py, width 2, MerkleHasher_MiMC: level 0 holds the leaves, node j of level d + 1 is
//     mimc_hash([n(d, 2j), n(d, 2j + 1)], IV[d])          (src/gadgets/mimc.hpp:352-393, merkletree.py:36-44)
// and with n leaves level d stores cnt_d = ceil(n / 2^d) nodes.  A node that does not exist reads as the placeholder
// unique(d, index) = sha256(be16(d) || be240(index)) mod r; extents are prefixes, so a level meets at most ONE placeholder, at index cnt_d,
// and only when cnt_d is odd.  The host keeps unique(d, cnt_d) for every level in a 29-element device table (TreeView::ph).
//
// One node = 2 ciphers x 91 rounds x (2 squarings + 2 products) = 728 Fr products on one dependent chain, VALU-bound like the rest of this
// code base.  Values are Montgomery and canonical ([0, r)) in memory; a hash runs in the loose domain of bn254.hpp and folds once at the end.
// The 91 round constants are read from a device table with a wave-uniform index: scalar loads, one copy per wave, no per-lane state.
//
// Kernels:
//   k_mimc_merkle_level   one lane per parent of a contiguous range of one level (bulk build, the levels wider than a workgroup)
//   k_mimc_merkle_update  the same for a sorted list of parent indices (batched update)
//   k_mimc_merkle_tail    ONE workgroup walks every remaining level, a barrier between two levels: the upper levels of a tree have fewer
//                         nodes than a workgroup has lanes and each costs a full chain latency however few nodes it has, so they share a launch
//   k_mtree_ingest        new leaves: range check (< r), canonical -> Montgomery
//   k_mtree_set_leaves    scatter updated leaves
//   k_mtree_gather        leaves and authentication paths of k indices (canonical, for the host)
//   k_mtree_fill_witness  the membership circuit's inputs of k indices, straight into k rows of a device witness buffer
//   k_mtree_fill_levels   the rest of that row: one lane per (row, level) writes the level's selector and hash variables (both hashers)
//   k_mtree_useq_*        ordered leaf updates, each seen by its successors, with the witnesses of the update circuit (both hashers): the k
//                         chains advance one level per step (_tail: every level in one workgroup, _level: one launch per level), then one lane
//                         per (row, level, side) traces the old and the new chain (_fill_inputs, _fill_levels), then _commit writes the tree
//   k_mimc_hash2          n independent two-block hashes (test entry point)
//
// The same tree over the Poseidon hasher (MerkleHasher_Poseidon, merkletree.py:63-78; the permutation is poseidon.hpp) has node widths
// w = 2, 3, 4: node j of level d + 1 is poseidon([n(d, w j), .., n(d, w j + w - 1)]) -- no IV, the depth does not enter the hash -- and level d
// stores cnt_d = ceil(n / w^d) nodes.  The last parent of a level can meet up to w - 1 absent children, at indices cnt_d .. (next multiple of
// w) - 1, so the placeholder table holds w - 1 entries per level: ph[d (w - 1) + k] = unique(d, cnt_d + k).  (w = 2: the MiMC table.)
//   k_poseidon_merkle_level / _update / _tail    the three hashing kernels above, for the Poseidon hasher; the width is a wave-uniform value
// The kernels that move leaves and paths serve both hashers.
#pragma once
#include "bn254.hpp"
#include "mimc.hpp"
#include "poseidon.hpp"

namespace zk {
namespace merkle {

constexpr uint32_t MAX_DEPTH = 29;                              // the gadget's IV table has 29 entries (merkle_tree_IVs)
constexpr uint32_t MAX_WIDTH = 4;                               // Poseidon nodes: 2, 3 or 4 children (merkletree.py:68 with t = 6)
constexpr uint32_t LEVEL_BLOCK = 64;
constexpr uint32_t TAIL_BLOCK = 256;                            // a level with at most this many parents goes through the tail kernel

// Miyaguchi-Preneel over two blocks: k1 = iv + E_iv(l) + l, k2 = k1 + E_k1(r) + r; canonical result
ZK_HD fe mimc_hash2(const fe *__restrict__ rc, const fe &l, const fe &r, const fe &iv) {
    const fe k1 = Fr::ladd(Fr::ladd(iv, mimc_cipher(rc, l, iv)), l);
    const fe k2 = Fr::ladd(Fr::ladd(k1, mimc_cipher(rc, r, k1)), r);
    return Fr::canon(k2);
}

// what every kernel knows of a tree: lvl[d] = the nodes of level d (d = 0 .. depth), ph[d (width - 1) + k] = unique(d, cnt_d + k), n = leaves,
// pc = the Poseidon constants (poseidon.hpp)
struct TreeView {
    fe *const *lvl;
    const fe *ph, *rc, *iv, *pc;
    uint64_t n;
    uint32_t depth, width;
};
ZK_HD uint64_t level_count(uint64_t n, uint32_t d) { return (n + (((uint64_t)1 << d) - 1)) >> d; }
// ceil(n / w^d) for w = 2, 3, 4 (a ceiling division taken d times is the ceiling division by w^d)
ZK_HD uint64_t level_count_w(uint64_t n, uint32_t d, uint32_t w) {
    if (w == 2) return level_count(n, d);
    if (w == 4) return level_count(n, 2 * d);
    for (uint32_t i = 0; i < d; i++) n = (n + w - 1) / w;
    return n;
}
ZK_HD uint64_t pow_w(uint32_t w, uint32_t e) { uint64_t p = 1; for (uint32_t i = 0; i < e; i++) p *= w; return p; }

// parent j of child level d (the caller guarantees 2 j < cnt_d)
ZK_D void hash_parent(const TreeView &t, uint32_t d, uint64_t j) {
    const fe *__restrict__ child = t.lvl[d];
    const uint64_t cnt = level_count(t.n, d);
    const fe l = child[2 * j];
    const fe r = 2 * j + 1 < cnt ? child[2 * j + 1] : t.ph[d];
    t.lvl[d + 1][j] = mimc_hash2(t.rc, l, r, t.iv[d]);
}

__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mimc_merkle_level(TreeView t, uint32_t d, uint64_t j0, uint64_t nj) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nj) return;
    hash_parent(t, d, j0 + g);
}

__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mimc_merkle_update(TreeView t, uint32_t d, const uint64_t *__restrict__ list, uint32_t nj) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nj) return;
    hash_parent(t, d, list[g]);
}

// child levels d_begin .. depth - 1 in one workgroup.  lists == nullptr: the parents of level d + 1 that cover the leaves s_old .. n - 1
// (an append); else row d of lists (stride entries apart) holds nlist[d] parent indices (an update).  Every level has at most blockDim.x
// parents (the host checks); the barrier makes level d + 1 visible to the lanes that hash level d + 2 from it.
__global__ void __launch_bounds__(TAIL_BLOCK)
k_mimc_merkle_tail(TreeView t, uint32_t d_begin, uint64_t s_old, const uint64_t *__restrict__ lists, const uint32_t *__restrict__ nlist, uint32_t stride) {
    for (uint32_t d = d_begin; d < t.depth; d++) {
        uint64_t j; bool on;
        if (lists) { on = threadIdx.x < nlist[d]; j = on ? lists[(size_t)d * stride + threadIdx.x] : 0; }
        else { const uint64_t j0 = s_old >> (d + 1); j = j0 + threadIdx.x; on = j < level_count(t.n, d + 1); }
        if (on) hash_parent(t, d, j);
        __syncthreads();
    }
}

// ---- the Poseidon hasher.  Parent j of child level d (the caller guarantees w j < cnt_d): its children, placeholders where the level ends
ZK_D void poseidon_hash_parent(const TreeView &t, uint32_t d, uint64_t j) {
    const fe *__restrict__ child = t.lvl[d];
    const uint32_t w = t.width;
    const uint64_t cnt = level_count_w(t.n, d, w);
    fe x[poseidon::T];
#pragma unroll
    for (uint32_t k = 0; k < poseidon::T; k++) {
        const uint64_t c = j * w + k;
        x[k] = k >= w ? Fr::zero() : c < cnt ? child[c] : t.ph[(size_t)d * (w - 1) + (c - cnt)];
    }
    poseidon::permute<poseidon::POSEIDON_MIX_DOT6>(t.pc, x);
    t.lvl[d + 1][j] = Fr::canon(x[0]);
}

__global__ void __launch_bounds__(LEVEL_BLOCK)
k_poseidon_merkle_level(TreeView t, uint32_t d, uint64_t j0, uint64_t nj) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nj) return;
    poseidon_hash_parent(t, d, j0 + g);
}

__global__ void __launch_bounds__(LEVEL_BLOCK)
k_poseidon_merkle_update(TreeView t, uint32_t d, const uint64_t *__restrict__ list, uint32_t nj) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nj) return;
    poseidon_hash_parent(t, d, list[g]);
}

// as k_mimc_merkle_tail; an append re-hashes on level d + 1 the parents s_old / w^(d+1) .. cnt_{d+1} - 1
__global__ void __launch_bounds__(TAIL_BLOCK)
k_poseidon_merkle_tail(TreeView t, uint32_t d_begin, uint64_t s_old, const uint64_t *__restrict__ lists, const uint32_t *__restrict__ nlist, uint32_t stride) {
    uint64_t pw = pow_w(t.width, d_begin + 1);
    for (uint32_t d = d_begin; d < t.depth; d++, pw *= t.width) {
        uint64_t j; bool on;
        if (lists) { on = threadIdx.x < nlist[d]; j = on ? lists[(size_t)d * stride + threadIdx.x] : 0; }
        else { j = s_old / pw + threadIdx.x; on = j < level_count_w(t.n, d + 1, t.width); }
        if (on) poseidon_hash_parent(t, d, j);
        __syncthreads();
    }
}

// leaves in place: bad += 1 for every value >= r (such a value is left as it is); canonical != 0: to Montgomery form
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_ingest(fe *__restrict__ x, uint64_t n, int canonical, uint32_t *__restrict__ bad) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const fe v = x[g];
    if (!fr_lt_modulus(v)) { atomicAdd(bad, 1u); return; }
    if (canonical) x[g] = Fr::to_mont(v);
}

// lvl[0][idx[i]] = vals[i] (Montgomery, already checked; the host removed duplicate indices)
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_set_leaves(TreeView t, const uint64_t *__restrict__ idx, const fe *__restrict__ vals, uint32_t k) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= k) return;
    t.lvl[0][idx[g]] = vals[g];
}

// node (d, o) as a path reads it: the stored node or one of the level's placeholders (cnt_d <= o < cnt_d + width - 1 then)
ZK_D fe node_or_placeholder(const TreeView &t, uint32_t d, uint64_t o) {
    const uint64_t cnt = level_count_w(t.n, d, t.width);
    return o < cnt ? t.lvl[d][o] : t.ph[(size_t)d * (t.width - 1) + (o - cnt)];
}

// one lane per (index, slot): slot 0 = the leaf -> leaves[i], slot 1 + d (w - 1) + q = sibling q of level d -> paths[(i depth + d)(w - 1) + q];
// the siblings of a level are the other nodes of the own parent in node order (merkletree.py:163-177).  Canonical values
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_gather(TreeView t, const uint64_t *__restrict__ idx, uint32_t k, fe *__restrict__ leaves, fe *__restrict__ paths) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t w = t.width, P = t.depth * (w - 1), S = P + 1;
    if (g >= (uint64_t)k * S) return;
    const uint32_t i = (uint32_t)(g / S), s = (uint32_t)(g % S);
    const uint64_t a = idx[i];
    if (s == 0) { leaves[i] = Fr::from_mont(t.lvl[0][a]); return; }
    const uint32_t d = (s - 1) / (w - 1), q = (s - 1) % (w - 1);
    const uint64_t ad = a / pow_w(w, d);                         // the own node on level d
    const uint32_t own = (uint32_t)(ad % w);
    paths[(size_t)i * P + (s - 1)] = Fr::from_mont(node_or_placeholder(t, d, ad - own + (q < own ? q : q + 1)));
}

// where the membership circuit keeps its inputs in a witness row (variable indices; zk_mtree_layout of include/zkhip.h)
struct Layout { uint32_t root_var, addr_var0, path_var0, leaf_var, iv_var0, n_iv; };

// one lane per (row, slot): ONE, the root, depth address bits, depth path elements, the leaf, n_iv IVs.  Nothing else of the row is written.
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_fill_witness(TreeView t, const uint64_t *__restrict__ idx, uint32_t k, fe *__restrict__ w, uint64_t row_elems, Layout L) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t D = t.depth, S = 3 + 2 * D + L.n_iv;
    if (g >= (uint64_t)k * S) return;
    const uint32_t i = (uint32_t)(g / S);
    uint32_t s = (uint32_t)(g % S);
    const uint64_t a = idx[i];
    fe *__restrict__ row = w + (size_t)i * row_elems;
    if (s == 0) { row[0] = Fr::one(); return; }
    if (s == 1) { row[L.root_var] = t.lvl[D][0]; return; }
    s -= 2;
    if (s < D) { row[L.addr_var0 + s] = ((a >> s) & 1) ? Fr::one() : Fr::zero(); return; }
    s -= D;
    if (s < D) { row[L.path_var0 + s] = node_or_placeholder(t, s, (a >> s) ^ 1); return; }
    s -= D;
    if (s == 0) { row[L.leaf_var] = t.lvl[0][a]; return; }
    row[L.iv_var0 + (s - 1)] = t.iv[s - 1];
}

// ---- complete membership witnesses.  Every node of a path is in the tree already, so the D levels of one witness do not wait for each other:
// one lane per (row, level) reads its own node x = lvl[d][a >> d] and the sibling p, and writes the level's variables in the gadgets'
// allocation order at row[level_var0 + d level_stride ..]: the six of merkle_path_selector, then the intermediates of ONE ordinary hash.
// Every stored value is canonical.  A lane streams its 322 or 736 elements as 32-byte stores to consecutive addresses (whole sectors; the
// lines fill up in L2); its depth is one hash, whatever the size of the circuit.
constexpr uint32_t SELECTOR_VARS = 6;
constexpr uint32_t POSEIDON_LEVEL_VARS = SELECTOR_VARS + 3 * poseidon::N_SBOX + 1;            // 322: selector, S-boxes, output
constexpr uint32_t MIMC_LEVEL_VARS = SELECTOR_VARS + 2 + 2 * 4 * MIMC_ROUNDS;                  // 736: selector, outputs[0..1], 2 x 91 x (a, b, c, d)

// left_a, left_b, left, right_a, right_b, right (MerklePathSelector) for a bit that is 0 or 1: products by the bit are selections
ZK_HD fe select(bool c, const fe &a, const fe &b) {              // limb by limb: a choice between two structs would go through memory
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
ZK_HD void store_selector(fe *__restrict__ o, bool bit, const fe &x, const fe &p, fe &left, fe &right) {
    const fe z = Fr::zero();
    left = select(bit, p, x); right = select(bit, x, p);
    o[0] = select(bit, z, x); o[1] = select(bit, p, z); o[2] = left;
    o[3] = select(bit, x, z); o[4] = select(bit, z, p); o[5] = right;
}

// MiMC_e7_gadget over message x0 with key k: (a, b, c, d) of every round at o[4 i ..], canonical; returns the loose result (the last d)
ZK_HD fe mimc_cipher_traced(const fe *__restrict__ rc, const fe &x0, const fe &k, fe *__restrict__ o) {
    fe x = x0;
    for (uint32_t i = 0; i < MIMC_ROUNDS; i++) {
        const fe t = Fr::ladd(Fr::ladd(x, k), rc[i]);
        const fe a = Fr::lsqr(t);
        const fe b = Fr::lsqr(a);
        const fe c = Fr::lmul(a, b);
        x = Fr::lmul(c, t);
        if (i + 1 == MIMC_ROUNDS) x = Fr::ladd(x, k);
        o[4 * i] = Fr::canon(a); o[4 * i + 1] = Fr::canon(b); o[4 * i + 2] = Fr::canon(c); o[4 * i + 3] = Fr::canon(x);
    }
    return x;
}

// the variables of one level at o[0 .. 321 / 735]: the selector of own node x and sibling p under the address bit, then the hash of (left, right)
template <bool POSEIDON>
ZK_D void trace_level(const TreeView &t, uint32_t d, bool bit, const fe &x, const fe &p, fe *__restrict__ o) {
    fe left, right;
    store_selector(o, bit, x, p, left, right);
    o += SELECTOR_VARS;
    if constexpr (POSEIDON) {
        fe s[poseidon::T] = {left, right, Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
        poseidon::permute_traced<poseidon::POSEIDON_MIX_DOT6>(t.pc, s, o);
        o[3 * poseidon::N_SBOX] = Fr::canon(s[0]);
    } else {
        const fe iv = t.iv[d];
        const fe k1 = Fr::ladd(Fr::ladd(iv, mimc_cipher_traced(t.rc, left, iv, o + 2)), left);
        o[0] = Fr::canon(k1);
        const fe k2 = Fr::ladd(Fr::ladd(k1, mimc_cipher_traced(t.rc, right, k1, o + 2 + 4 * MIMC_ROUNDS)), right);
        o[1] = Fr::canon(k2);
    }
}

template <bool POSEIDON>
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_fill_levels(TreeView t, const uint64_t *__restrict__ idx, uint32_t k, fe *__restrict__ w, uint64_t row_elems, uint32_t level_var0, uint32_t level_stride) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t D = t.depth;
    if (g >= (uint64_t)k * D) return;
    const uint32_t i = (uint32_t)(g / D), d = (uint32_t)(g % D);
    const uint64_t ad = idx[i] >> d;                             // the own node on level d
    trace_level<POSEIDON>(t, d, ad & 1, t.lvl[d][ad], node_or_placeholder(t, d, ad ^ 1), w + (size_t)i * row_elems + level_var0 + (size_t)d * level_stride);
}

// ---- ordered leaf updates with transition witnesses (zk_mtree_update_seq).  Update j of k replaces leaf a_j and is seen by every later update.
// With n(d, j) = a_j >> d:  N[d][j] = node n(d, j) after update j (N[0][j] = the new leaf), S[d][j] = its sibling as update j sees it,
// O[d][j] = the own node before update j.  S[d][j] = N[d][i] for the largest i < j with n(d, i) = n(d, j) ^ 1, O[d][j] likewise with
// n(d, i) = n(d, j); without such an i they are what the tree holds.  N[d + 1][j] = H(N[d][j], S[d][j]) ordered by the address bit: level d + 1
// needs level d of EVERY update and nothing else, so the k chains advance together and the call costs D dependent hashes, not k D.
// The host finds the predecessors (UpdateSeq::pred_same, pred_sib: i or -1; last: update j is the last that touches n(d, j)); nodes is the
// (D + 1) x k scratch N, level major.  Only k_mtree_useq_commit writes the tree.
struct UpdateSeq {
    const uint64_t *idx;                                        // k leaf indices
    const int32_t *pred_same, *pred_sib;                        // D x k
    const uint8_t *last;                                        // (D + 1) x k
    fe *nodes;                                                  // (D + 1) x k, row 0 = the new leaves (Montgomery)
    uint32_t k;
};
ZK_D fe useq_sibling(const TreeView &t, const UpdateSeq &u, uint32_t d, uint32_t j) {
    const int32_t i = u.pred_sib[(size_t)d * u.k + j];
    return i >= 0 ? u.nodes[(size_t)d * u.k + i] : node_or_placeholder(t, d, (u.idx[j] >> d) ^ 1);
}
ZK_D fe useq_own_before(const TreeView &t, const UpdateSeq &u, uint32_t d, uint32_t j) {
    const int32_t i = u.pred_same[(size_t)d * u.k + j];
    return i >= 0 ? u.nodes[(size_t)d * u.k + i] : t.lvl[d][u.idx[j] >> d];
}
template <bool POSEIDON>
ZK_D void useq_step(const TreeView &t, const UpdateSeq &u, uint32_t d, uint32_t j) {
    const bool bit = (u.idx[j] >> d) & 1;
    const fe x = u.nodes[(size_t)d * u.k + j], p = useq_sibling(t, u, d, j);
    const fe l = select(bit, p, x), r = select(bit, x, p);
    fe out;
    if constexpr (POSEIDON) {
        fe s[poseidon::T] = {l, r, Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
        poseidon::permute<poseidon::POSEIDON_MIX_DOT6>(t.pc, s);
        out = Fr::canon(s[0]);
    } else out = mimc_hash2(t.rc, l, r, t.iv[d]);
    u.nodes[(size_t)(d + 1) * u.k + j] = out;
}

// phase 1, k > TAIL_BLOCK: one launch per level, one lane per update
template <bool POSEIDON>
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_useq_level(TreeView t, UpdateSeq u, uint32_t d) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < u.k) useq_step<POSEIDON>(t, u, d, j);
}

// phase 1, k <= TAIL_BLOCK: every level in ONE workgroup, as k_mimc_merkle_tail; the barrier makes level d + 1 of every update visible
template <bool POSEIDON>
__global__ void __launch_bounds__(TAIL_BLOCK)
k_mtree_useq_tail(TreeView t, UpdateSeq u) {
    for (uint32_t d = 0; d < t.depth; d++) {
        if (threadIdx.x < u.k) useq_step<POSEIDON>(t, u, d, threadIdx.x);
        __syncthreads();
    }
}

// where the update circuit keeps its inputs in a witness row (zk_mtree_update_layout of include/zkhip.h)
struct UpdateLayout { uint32_t old_root_var, new_root_var, addr_var0, path_var0, old_leaf_var, new_leaf_var, iv_var0, n_iv; };

// phase 2a, one lane per (row, slot): ONE, the two roots, depth address bits, depth path elements, the two leaves, n_iv IVs
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_useq_fill_inputs(TreeView t, UpdateSeq u, fe *__restrict__ w, uint64_t row_elems, UpdateLayout L) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t D = t.depth, S = 5 + 2 * D + L.n_iv;
    if (g >= (uint64_t)u.k * S) return;
    const uint32_t j = (uint32_t)(g / S);
    uint32_t s = (uint32_t)(g % S);
    fe *__restrict__ row = w + (size_t)j * row_elems;
    if (s == 0) { row[0] = Fr::one(); return; }
    if (s == 1) { row[L.old_root_var] = j ? u.nodes[(size_t)D * u.k + (j - 1)] : t.lvl[D][0]; return; }
    if (s == 2) { row[L.new_root_var] = u.nodes[(size_t)D * u.k + j]; return; }
    s -= 3;
    if (s < D) { row[L.addr_var0 + s] = ((u.idx[j] >> s) & 1) ? Fr::one() : Fr::zero(); return; }
    s -= D;
    if (s < D) { row[L.path_var0 + s] = useq_sibling(t, u, s, j); return; }
    s -= D;
    if (s == 0) { row[L.old_leaf_var] = useq_own_before(t, u, 0, j); return; }
    if (s == 1) { row[L.new_leaf_var] = u.nodes[j]; return; }
    row[L.iv_var0 + (s - 2)] = t.iv[s - 2];
}

// phase 2b, one lane per (row, level, side): the level's variables of the old chain (own node O[d][j]) at level_var0 + d level_stride, of the
// new chain (own node N[d][j]) at level_var0 + (D + d) level_stride; both over the sibling S[d][j].  No lane waits for another
template <bool POSEIDON>
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_useq_fill_levels(TreeView t, UpdateSeq u, fe *__restrict__ w, uint64_t row_elems, uint32_t level_var0, uint32_t level_stride) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t D = t.depth;
    if (g >= (uint64_t)u.k * D * 2) return;
    const uint32_t j = (uint32_t)(g / (2 * D)), d = (uint32_t)(g % (2 * D)) >> 1;
    const bool is_new = g & 1;
    const fe x = is_new ? u.nodes[(size_t)d * u.k + j] : useq_own_before(t, u, d, j);
    trace_level<POSEIDON>(t, d, (u.idx[j] >> d) & 1, x, useq_sibling(t, u, d, j),
                          w + (size_t)j * row_elems + level_var0 + (size_t)((is_new ? D : 0) + d) * level_stride);
}

// phase 3, one lane per (update, level 0 .. D): the last update that touches a node stores it
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mtree_useq_commit(TreeView t, UpdateSeq u) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)u.k * (t.depth + 1)) return;
    const uint32_t d = (uint32_t)(g / u.k), j = (uint32_t)(g % u.k);
    if (u.last[g]) t.lvl[d][u.idx[j] >> d] = u.nodes[g];
}

// out[i] = mimc_hash([l[i], r[i]], iv[i]); canonical in and out (the host has checked the operands against r)
__global__ void __launch_bounds__(LEVEL_BLOCK)
k_mimc_hash2(const fe *__restrict__ l, const fe *__restrict__ r, const fe *__restrict__ iv, uint32_t n, const fe *__restrict__ rc, fe *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    out[g] = Fr::from_mont(mimc_hash2(rc, Fr::to_mont(l[g]), Fr::to_mont(r[g]), Fr::to_mont(iv[g])));
}

}  // namespace merkle
}  // namespace zk
