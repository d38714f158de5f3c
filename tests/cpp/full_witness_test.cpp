// tests/cpp/full_witness_test.cpp -- ethsnarks::MerkleTreeHIP::fill_full_witnesses (include/ethsnarks_hip/merkle.hpp) against the witness of the
// C++ gadgets of include/ethsnarks_hip/gadgets.hpp: the membership circuit of every leaf of a small tree is built on the host from the tree's own
// proof, and the rows the device wrote must be its pb.values byte for byte (both are 4 x u64 Montgomery limbs, ONE at index 0).  Compiled by
// tests/test_full_witness_cpp.py against the CPU emulation build and by tests/test_full_witness_gpu.py against libzkhip.so.
//
//   full_witness_test <mimc|poseidon> <depth> <leaf_0> <leaf_1> ..      field values as decimal numerals                       prints FULL OK
#include "ethsnarks_hip/gadgets.hpp"
#include "ethsnarks_hip/merkle.hpp"

#include <cstring>
#include <iostream>

using namespace ethsnarks;

#define EXPECT(cond) do { if (!(cond)) { std::cerr << "failed: " #cond << std::endl; return 1; } } while (0)

static_assert(sizeof(FieldT) == 32, "a FieldT is the 32-byte Montgomery image the device writes");

static zk_fr to_fr(const FieldT &v) { const FieldT::bigint b = v.as_bigint(); return zk_fr{b.data[0], b.data[1], b.data[2], b.data[3]}; }
static FieldT from_fr(const zk_fr &v) { FieldT::bigint b; for (int i = 0; i < 4; i++) b.data[i] = v[(size_t)i]; return FieldT(b); }

// the membership circuit's witness for one proof, in the allocation order root, address bits, path, leaf, (29 IVs,) levels
static int host_witness(bool poseidon_tree, size_t depth, uint64_t address, const MerkleProofHIP &proof, const zk_fr &root, std::vector<FieldT> &out) {
    ProtoboardT pb;
    const VariableT root_var = make_variable(pb, from_fr(root), "root");
    pb.set_input_sizes(1);
    const VariableArrayT bits = make_var_array(pb, depth, "address"), path = make_var_array(pb, depth, "path");
    const VariableT leaf = make_variable(pb, from_fr(proof.leaf), "leaf");
    bits.fill_with_bits_of_ulong(pb, address);
    for (size_t d = 0; d < depth; d++) pb.val(path[d]) = from_fr(proof.path[d]);
    if (poseidon_tree) {
        std::vector<std::unique_ptr<merkle_path_selector>> selectors;
        std::vector<std::unique_ptr<Poseidon128<2, 1>>> hashers;
        VariableT item = leaf;
        for (size_t d = 0; d < depth; d++) {
            selectors.emplace_back(new merkle_path_selector(pb, item, path[d], bits[d], FMT("", ".selector[%zu]", d)));
            VariableArrayT lr;
            lr.push_back(selectors[d]->left()); lr.push_back(selectors[d]->right());
            hashers.emplace_back(new Poseidon128<2, 1>(pb, lr, FMT("", ".hasher[%zu]", d)));
            selectors[d]->generate_r1cs_witness(); hashers[d]->generate_r1cs_witness();
            selectors[d]->generate_r1cs_constraints(); hashers[d]->generate_r1cs_constraints();
            item = hashers[d]->result();
        }
        pb.add_r1cs_constraint(ConstraintT(item, 1, root_var), "result = root");
        EXPECT(pb.num_constraints() == 322 * depth + 1);
    } else {
        const VariableArrayT ivs = merkle_tree_IVs(pb);
        merkle_path_authenticator<MiMC_e7_hash_gadget> auth(pb, depth, bits, ivs, leaf, root_var, path, "auth");
        auth.generate_r1cs_witness();
        auth.generate_r1cs_constraints();
        EXPECT(auth.is_valid() && pb.num_constraints() == 736 * depth + 1);
    }
    EXPECT(pb.is_satisfied());
    out = pb.values;
    return 0;
}

static int run(int argc, char **argv) {
    const bool poseidon_tree = std::string(argv[1]) == "poseidon";
    const uint32_t depth = (uint32_t)std::stoul(argv[2]);
    std::vector<zk_fr> leaves;
    for (int i = 3; i < argc; i++) leaves.push_back(to_fr(FieldT(argv[i])));
    const size_t n = leaves.size();
    MerkleTreeHIP t(depth, 2, poseidon_tree ? MerkleHasher::Poseidon : MerkleHasher::MiMC);
    t.extend(leaves);
    EXPECT(t.level_stride() == (poseidon_tree ? 322u : 736u) && t.level_var0() == 3 + 2 * depth + (poseidon_tree ? 0u : 29u));
    const uint64_t elems = t.full_row_elems();
    std::vector<uint64_t> all;
    for (uint64_t i = 0; i < n; i++) all.push_back(n - 1 - i);  // not in leaf order
    const std::vector<MerkleProofHIP> proofs = t.proofs(all);
    // n rows and one more that must stay as it is
    std::vector<uint64_t> sentinel((n + 1) * elems * 4), got(sentinel.size());
    for (size_t i = 0; i < sentinel.size(); i++) sentinel[i] = 7 + i;
    void *d_w = nullptr;
    EXPECT(zk_dev_alloc(sentinel.size() * 8, 0, &d_w) == ZK_OK);
    EXPECT(zk_dev_upload(d_w, sentinel.data(), sentinel.size() * 8) == ZK_OK);
    t.fill_full_witnesses(all, d_w, elems);
    EXPECT(zk_dev_download(got.data(), d_w, got.size() * 8) == ZK_OK);
    for (size_t p = 0; p < n; p++) {
        std::vector<FieldT> w;
        if (host_witness(poseidon_tree, depth, all[p], proofs[p], t.root(), w)) return 1;
        EXPECT(w.size() == elems);
        EXPECT(!memcmp(w.data(), got.data() + p * elems * 4, elems * 32));
    }
    EXPECT(!memcmp(sentinel.data() + n * elems * 4, got.data() + n * elems * 4, elems * 32));
    // a refused call throws and leaves the buffer alone; no indices: nothing happens
    bool threw = false;
    try { t.fill_full_witnesses({n}, d_w, elems); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG && std::string(e.what()).size() > 0; }
    EXPECT(threw);
    threw = false;
    try { t.fill_full_witnesses({0}, d_w, elems - 1); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);
    t.fill_full_witnesses({}, d_w, elems);
    std::vector<uint64_t> again(got.size());
    EXPECT(zk_dev_download(again.data(), d_w, again.size() * 8) == ZK_OK && again == got);
    EXPECT(zk_dev_free(d_w) == ZK_OK);
    std::cout << "FULL OK" << std::endl;
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc >= 5 && (std::string(argv[1]) == "mimc" || std::string(argv[1]) == "poseidon")) return run(argc, argv);
        std::cerr << "usage: " << argv[0] << " mimc|poseidon <depth> <leaf_0> <leaf_1> .." << std::endl;
        return 2;
    } catch (const std::exception &e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
}
