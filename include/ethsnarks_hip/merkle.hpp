// ethsnarks_hip/merkle.hpp -- the device MiMC Merkle tree of libzkhip.so (zk_mtree_* of zkhip.h) as a C++ object: the tree of the reference's
// ethsnarks/merkletree.py (width 2, MerkleHasher_MiMC) kept in GPU memory and hashed by HIP kernels.  Header-only, RAII, no libsnark types:
// a field element is a zk_fr = 4 x u64 little-endian limbs, canonical (not Montgomery) wherever it crosses this interface.
//
//   ethsnarks::MerkleTreeHIP tree(29);                 depth 1 .. 29, capacity 2^depth
//   tree.append(leaf); tree.extend(leaves); tree.update(i, leaf); tree.update_many(indices, leaves);
//   tree.size(); tree.empty(); tree.root();            root() throws on an empty tree (the reference's root is None then)
//   tree.node(level, offset);                          the reference's tree.leaf(depth, offset), placeholders included
//   tree.proof(i) / tree.proofs(indices);              leaf, address bits, path (level 0 first)
//   tree.fill_witnesses(indices, d_w, row_elems);      inputs of merkle_path_authenticator for k leaves into a device witness buffer, for
//                                                      zk_wplan_solve and zk_prove_batch_submit_resident
//   tree.fill_full_witnesses(indices, d_w, row_elems); the COMPLETE witness of the membership circuit instead (selector and hash variables of
//                                                      every level, computed from the tree's nodes): nothing is left for zk_wplan_solve
//   tree.update_seq(indices, leaves, d_w, row_elems);  ORDERED updates (an index may repeat; each sees its predecessors): returns the k + 1 roots
//                                                      before / after every update, and with d_w != nullptr writes per update the complete
//                                                      witness of the update circuit (two markle_path_compute over one path: old leaf ->
//                                                      old root, new leaf -> new root); width 2 only
//   ethsnarks::MerkleTreeHIP wide(14, 4, MerkleHasher::Poseidon);   the same tree over Poseidon128, node width 2, 3 or 4 (capacity width^depth
//                                                      <= 2^29); a proof then carries `digits` and width - 1 siblings per level in `path`
// Every failure is a mtree_error carrying the C ABI's code and zk_last_error()'s text.
#pragma once
#include <zkhip.h>

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace ethsnarks {

typedef std::array<uint64_t, 4> zk_fr;

struct mtree_error : std::runtime_error {
    int code;
    explicit mtree_error(int c) : std::runtime_error(std::string(zk_strerror(c)) + ": " + zk_last_error()), code(c) {}
};

enum class MerkleHasher { MiMC = ZK_MTREE_HASH_MIMC, Poseidon = ZK_MTREE_HASH_POSEIDON };

struct MerkleProofHIP {
    zk_fr leaf;
    std::vector<bool> address;                                   // width 2 -- bit d: the node is the right child on level d
    std::vector<uint32_t> digits;                                // any width: the node's position among the children of its parent on level d
    std::vector<zk_fr> path;                                     // width - 1 siblings per level, level 0 first, in node order
};

class MerkleTreeHIP {
    zk_mtree *h_ = nullptr;
    uint32_t depth_ = 0, width_ = 2;
    MerkleHasher hasher_ = MerkleHasher::MiMC;
    static void check(int rc) { if (rc != ZK_OK) throw mtree_error(rc); }

public:
    explicit MerkleTreeHIP(uint32_t depth, uint64_t reserve_leaves = 0, int device = 0) : depth_(depth) { check(zk_mtree_create(depth, reserve_leaves, device, &h_)); }
    MerkleTreeHIP(uint32_t depth, uint32_t width, MerkleHasher hasher, uint64_t reserve_leaves = 0, int device = 0) : depth_(depth), width_(width), hasher_(hasher) {
        check(zk_mtree_create_ex(depth, width, (int)hasher, reserve_leaves, device, &h_));
    }
    ~MerkleTreeHIP() { zk_mtree_free(h_); }
    MerkleTreeHIP(const MerkleTreeHIP &) = delete;
    MerkleTreeHIP &operator=(const MerkleTreeHIP &) = delete;
    MerkleTreeHIP(MerkleTreeHIP &&o) noexcept : h_(o.h_), depth_(o.depth_), width_(o.width_), hasher_(o.hasher_) { o.h_ = nullptr; }

    uint32_t depth() const { return depth_; }
    uint32_t width() const { return width_; }
    MerkleHasher hasher() const { return hasher_; }
    uint64_t size() const { uint64_t n = 0; check(zk_mtree_size(h_, &n)); return n; }
    bool empty() const { return size() == 0; }
    zk_mtree *handle() const { return h_; }

    uint64_t append(const zk_fr &leaf) { const uint64_t i = size(); check(zk_mtree_append(h_, leaf.data(), 1, 1)); return i; }
    void extend(const std::vector<zk_fr> &leaves) { if (!leaves.empty()) check(zk_mtree_append(h_, leaves[0].data(), leaves.size(), 1)); }
    // n field elements already in device memory (Montgomery unless canonical)
    void extend_resident(const void *d_leaves, uint64_t n, bool canonical = false) { check(zk_mtree_append_resident(h_, d_leaves, n, canonical ? 1 : 0)); }
    void update(uint64_t index, const zk_fr &leaf) { check(zk_mtree_update(h_, &index, leaf.data(), 1, 1)); }
    // an index that occurs more than once takes the value of its last occurrence
    void update_many(const std::vector<uint64_t> &indices, const std::vector<zk_fr> &leaves) {
        if (indices.size() != leaves.size()) throw std::invalid_argument("update_many: indices and leaves differ in length");
        if (!indices.empty()) check(zk_mtree_update(h_, indices.data(), leaves[0].data(), (uint32_t)indices.size(), 1));
    }

    zk_fr root() const { zk_fr r; check(zk_mtree_root(h_, r.data())); return r; }
    zk_fr node(uint32_t level, uint64_t offset) const { zk_fr r; check(zk_mtree_node(h_, level, offset, r.data())); return r; }
    std::vector<MerkleProofHIP> proofs(const std::vector<uint64_t> &indices) const {
        const size_t k = indices.size();
        std::vector<MerkleProofHIP> out(k);
        if (!k) return out;
        const size_t per = (size_t)depth_ * (width_ - 1);
        std::vector<zk_fr> leaves(k), paths(k * per);
        check(zk_mtree_paths(h_, indices.data(), (uint32_t)k, leaves[0].data(), paths[0].data()));
        for (size_t j = 0; j < k; j++) {
            out[j].leaf = leaves[j];
            out[j].path.assign(paths.begin() + (long)(j * per), paths.begin() + (long)((j + 1) * per));
            uint64_t a = indices[j];
            for (uint32_t d = 0; d < depth_; d++, a /= width_) {
                out[j].digits.push_back((uint32_t)(a % width_));
                if (width_ == 2) out[j].address.push_back(a & 1);
            }
        }
        return out;
    }
    MerkleProofHIP proof(uint64_t index) const { return proofs({index})[0]; }

    // the allocation order of merkle_path_authenticator: root, address bits, path, leaf, 29 IVs; the Poseidon circuit has no IV variables
    zk_mtree_layout membership_layout() const {
        if (hasher_ == MerkleHasher::Poseidon) return zk_mtree_layout{1, 2, 2 + depth_, 2 + 2 * depth_, 0, 0};
        return zk_mtree_layout{1, 2, 2 + depth_, 2 + 2 * depth_, 3 + 2 * depth_, 29};
    }
    void fill_witnesses(const std::vector<uint64_t> &indices, void *d_w, uint64_t row_elems) const { fill_witnesses(indices, d_w, row_elems, membership_layout()); }
    void fill_witnesses(const std::vector<uint64_t> &indices, void *d_w, uint64_t row_elems, const zk_mtree_layout &layout) const {
        if (!indices.empty()) check(zk_mtree_fill_witnesses(h_, indices.data(), (uint32_t)indices.size(), d_w, row_elems, &layout));
    }

    // the complete witness: per level the six selector variables and the hash gadget's, 736 (MiMC) or 322 (Poseidon), after the inputs
    uint32_t level_stride() const { return hasher_ == MerkleHasher::Poseidon ? 322 : 736; }
    uint32_t level_var0() const { return 3 + 2 * depth_ + membership_layout().n_iv; }
    uint64_t full_row_elems() const { return (uint64_t)level_var0() + (uint64_t)level_stride() * depth_; }
    void fill_full_witnesses(const std::vector<uint64_t> &indices, void *d_w, uint64_t row_elems) const {
        fill_full_witnesses(indices, d_w, row_elems, membership_layout(), level_var0(), level_stride());
    }
    void fill_full_witnesses(const std::vector<uint64_t> &indices, void *d_w, uint64_t row_elems, const zk_mtree_layout &layout, uint32_t var0, uint32_t stride) const {
        if (!indices.empty()) check(zk_mtree_fill_full_witnesses(h_, indices.data(), (uint32_t)indices.size(), d_w, row_elems, &layout, var0, stride));
    }

    // ordered updates with the witnesses of the update circuit: old_root, new_root, address bits, path, old_leaf, new_leaf, (29 IVs,) then the
    // level blocks of the old chain and those of the new chain
    zk_mtree_update_layout update_layout() const {
        const uint32_t n_iv = membership_layout().n_iv;
        return zk_mtree_update_layout{1, 2, 3, 3 + depth_, 3 + 2 * depth_, 4 + 2 * depth_, n_iv ? 5 + 2 * depth_ : 0, n_iv};
    }
    uint32_t update_level_var0() const { return 5 + 2 * depth_ + membership_layout().n_iv; }
    uint64_t update_row_elems() const { return (uint64_t)update_level_var0() + 2 * (uint64_t)level_stride() * depth_; }
    // leaves[j] replaces leaf indices[j] in the given order; the k + 1 roots before and after every update.  d_w == nullptr: no witnesses
    std::vector<zk_fr> update_seq(const std::vector<uint64_t> &indices, const std::vector<zk_fr> &leaves, void *d_w = nullptr, uint64_t row_elems = 0) {
        return update_seq(indices, leaves, d_w, row_elems, update_layout(), update_level_var0(), level_stride());
    }
    std::vector<zk_fr> update_seq(const std::vector<uint64_t> &indices, const std::vector<zk_fr> &leaves, void *d_w, uint64_t row_elems,
                                  const zk_mtree_update_layout &layout, uint32_t var0, uint32_t stride) {
        if (indices.size() != leaves.size()) throw std::invalid_argument("update_seq: indices and leaves differ in length");
        if (indices.size() > 0x7fffffffu) throw std::invalid_argument("update_seq: more than 2^31 - 1 updates in one call");
        std::vector<zk_fr> roots(indices.size() + 1);
        check(zk_mtree_update_seq(h_, indices.data(), leaves.empty() ? nullptr : leaves[0].data(), (uint32_t)indices.size(), 1, d_w, row_elems, &layout, var0, stride,
                                  roots[0].data()));
        return roots;
    }
};

}  // namespace ethsnarks
