// tests/cpp/merkle_update_test.cpp -- ethsnarks::MerkleTreeHIP::update_seq (include/ethsnarks_hip/merkle.hpp): ordered leaf updates through the
// C++ wrapper.  The program applies the updates with a witness buffer, prints the k + 1 roots as decimal numerals (one per line) for the caller
// to compare, and checks what it can by itself: the two roots inside every witness row are the returned ones (Montgomery images, as FieldT
// holds them), the row after the last keeps its sentinel, a second tree given the same updates by single update() calls and a third by
// update_seq without a buffer end at the same root and leaves, and a refused call throws and changes nothing.  Compiled by
// tests/test_merkle_update_cpp.py against the CPU emulation build and by tests/test_merkle_update_gpu.py against libzkhip.so.
//
//   merkle_update_test <mimc|poseidon> <depth> <n> <k> <leaf_0> .. <leaf_{n-1}> <index_0> <value_0> .. <index_{k-1}> <value_{k-1}>
#include "ethsnarks_hip/gadgets.hpp"
#include "ethsnarks_hip/merkle.hpp"

#include <cstring>
#include <iostream>

using namespace ethsnarks;

#define EXPECT(cond) do { if (!(cond)) { std::cerr << "failed: " #cond << std::endl; return 1; } } while (0)

static_assert(sizeof(FieldT) == 32, "a FieldT is the 32-byte Montgomery image the device writes");

static zk_fr to_fr(const FieldT &v) { const FieldT::bigint b = v.as_bigint(); return zk_fr{b.data[0], b.data[1], b.data[2], b.data[3]}; }
static FieldT from_fr(const zk_fr &v) { FieldT::bigint b; for (int i = 0; i < 4; i++) b.data[i] = v[(size_t)i]; return FieldT(b); }

static int run(int argc, char **argv) {
    const bool poseidon_tree = std::string(argv[1]) == "poseidon";
    const uint32_t depth = (uint32_t)std::stoul(argv[2]);
    const size_t n = std::stoul(argv[3]), k = std::stoul(argv[4]);
    EXPECT((size_t)argc == 5 + n + 2 * k && k > 0);
    std::vector<zk_fr> leaves, values;
    std::vector<uint64_t> indices;
    for (size_t i = 0; i < n; i++) leaves.push_back(to_fr(FieldT(argv[5 + i])));
    for (size_t j = 0; j < k; j++) { indices.push_back(std::stoull(argv[5 + n + 2 * j])); values.push_back(to_fr(FieldT(argv[6 + n + 2 * j]))); }
    const MerkleHasher hasher = poseidon_tree ? MerkleHasher::Poseidon : MerkleHasher::MiMC;
    MerkleTreeHIP t(depth, 2, hasher), singles(depth, 2, hasher), bare(depth, 2, hasher);
    t.extend(leaves); singles.extend(leaves); bare.extend(leaves);
    const uint32_t n_iv = poseidon_tree ? 0u : 29u;
    EXPECT(t.update_level_var0() == 5 + 2 * depth + n_iv && t.update_row_elems() == t.update_level_var0() + 2ull * depth * t.level_stride());
    const zk_mtree_update_layout L = t.update_layout();
    EXPECT(L.old_root_var == 1 && L.new_root_var == 2 && L.addr_var0 == 3 && L.path_var0 == 3 + depth && L.old_leaf_var == 3 + 2 * depth && L.new_leaf_var == 4 + 2 * depth && L.n_iv == n_iv);
    const uint64_t elems = t.update_row_elems();
    std::vector<uint64_t> sentinel((k + 1) * elems * 4), got(sentinel.size());
    for (size_t i = 0; i < sentinel.size(); i++) sentinel[i] = 7 + i;
    void *d_w = nullptr;
    EXPECT(zk_dev_alloc(sentinel.size() * 8, 0, &d_w) == ZK_OK);
    EXPECT(zk_dev_upload(d_w, sentinel.data(), sentinel.size() * 8) == ZK_OK);
    // a refused call throws and leaves tree and buffer alone
    const zk_fr root0 = t.root();
    bool threw = false;
    try { t.update_seq({0, n}, {values[0], values[0]}, d_w, elems); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG && std::string(e.what()).size() > 0; }
    EXPECT(threw && t.root() == root0 && t.node(0, 0) == leaves[0]);
    threw = false;
    try { t.update_seq({0}, {values[0]}, d_w, elems - 1); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw && t.root() == root0 && t.node(0, 0) == leaves[0]);
    EXPECT(zk_dev_download(got.data(), d_w, got.size() * 8) == ZK_OK && got == sentinel);
    EXPECT(t.update_seq({}, {}) == std::vector<zk_fr>{root0});
    // the updates
    const std::vector<zk_fr> roots = t.update_seq(indices, values, d_w, elems);
    EXPECT(roots.size() == k + 1 && roots[0] == root0 && roots[k] == t.root());
    EXPECT(zk_dev_download(got.data(), d_w, got.size() * 8) == ZK_OK);
    for (size_t j = 0; j < k; j++) {
        const FieldT one = FieldT::one(), old_root = from_fr(roots[j]), new_root = from_fr(roots[j + 1]), new_leaf = from_fr(values[j]);
        const uint64_t *row = got.data() + j * elems * 4;
        EXPECT(!memcmp(row, &one, 32) && !memcmp(row + 4 * L.old_root_var, &old_root, 32) && !memcmp(row + 4 * L.new_root_var, &new_root, 32));
        EXPECT(!memcmp(row + 4 * L.new_leaf_var, &new_leaf, 32));
    }
    EXPECT(!memcmp(sentinel.data() + k * elems * 4, got.data() + k * elems * 4, elems * 32));
    for (size_t j = 0; j < k; j++) {
        singles.update(indices[j], values[j]);
        EXPECT(singles.root() == roots[j + 1]);
    }
    EXPECT(bare.update_seq(indices, values) == roots);
    for (uint64_t i = 0; i < n; i++) EXPECT(t.node(0, i) == singles.node(0, i) && t.node(0, i) == bare.node(0, i));
    for (uint32_t d = 1; d <= depth; d++) EXPECT(t.node(d, 0) == singles.node(d, 0) && t.node(d, 0) == bare.node(d, 0));
    EXPECT(zk_dev_free(d_w) == ZK_OK);
    for (const zk_fr &r : roots) std::cout << from_fr(r).to_decimal() << std::endl;
    std::cout << "UPDATE OK" << std::endl;
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc >= 8 && (std::string(argv[1]) == "mimc" || std::string(argv[1]) == "poseidon")) return run(argc, argv);
        std::cerr << "usage: " << argv[0] << " mimc|poseidon <depth> <n> <k> <leaf> .. <index> <value> .." << std::endl;
        return 2;
    } catch (const std::exception &e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
}
