// tests/cpp/merkle_tree_test.cpp -- ethsnarks::MerkleTreeHIP of the C++ adapter (include/ethsnarks_hip/merkle.hpp) on the reference's depth-29
// known answers (test/test_merkle.py:82-107); the driver passes them as 64-digit hex words so that this file holds no 254-bit literals.
// Compiled by tests/test_merkle_cpp.py against the CPU emulation build and by tests/test_merkle_gpu.py against libzkhip.so.
//
//   merkle_tree_test <item_a> <item_b> <root_after_a> <root_after_b> <node_13_1>     prints MTREE OK
#include "ethsnarks_hip/merkle.hpp"

#include <iostream>

using namespace ethsnarks;

static zk_fr parse(const char *hex) {
    const std::string s(hex);
    if (s.size() != 64) throw std::invalid_argument("expected 64 hex digits");
    zk_fr v;
    for (int i = 0; i < 4; i++) v[(size_t)i] = std::stoull(s.substr((size_t)(48 - 16 * i), 16), nullptr, 16);
    return v;
}
#define EXPECT(cond) do { if (!(cond)) { std::cerr << "failed: " #cond << std::endl; return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc != 6) { std::cerr << "usage: " << argv[0] << " <item_a> <item_b> <root_after_a> <root_after_b> <node_13_1>" << std::endl; return 2; }
    const zk_fr a = parse(argv[1]), b = parse(argv[2]), root_a = parse(argv[3]), root_b = parse(argv[4]), n13 = parse(argv[5]);
    MerkleTreeHIP tree(29);
    EXPECT(tree.empty());
    bool threw = false;
    try { tree.root(); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);                                               // an empty tree has no root
    EXPECT(tree.append(a) == 0);
    EXPECT(tree.root() == root_a);
    EXPECT(tree.append(b) == 1 && tree.size() == 2);
    EXPECT(tree.root() == root_b);
    EXPECT(tree.node(0, 0) == a && tree.node(13, 1) == n13);
    const MerkleProofHIP p = tree.proof(1);
    EXPECT(p.leaf == b && p.path.size() == 29 && p.path[0] == a && p.address[0] && !p.address[1] && p.path[13] == n13);
    // extend + update_many bring the tree back to the same root
    MerkleTreeHIP t2(29, 4);
    t2.extend({b, a});
    EXPECT(!(t2.root() == root_b));
    t2.update_many({0, 1, 1}, {a, a, b});                        // the last write to index 1 wins
    EXPECT(t2.root() == root_b);
    threw = false;
    try { t2.update(2, a); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);
    threw = false;
    try { MerkleTreeHIP bad(30); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);
    std::cout << "MTREE OK" << std::endl;
    return 0;
}
