// tests/cpp/poseidon_test.cpp -- the C++ Poseidon layer: FifthPower_gadget / Poseidon128 / poseidon() of include/ethsnarks_hip/gadgets.hpp and
// ethsnarks::MerkleTreeHIP with the Poseidon hasher (include/ethsnarks_hip/merkle.hpp).  Compiled by tests/test_poseidon_cpp.py against the CPU
// emulation build and by tests/test_poseidon_gpu.py against libzkhip.so; field values come in as decimal numerals.
//
//   poseidon_test kat                                             the reference's pinned values, gadget shapes                  prints OK
//   poseidon_test dump_gadget <r1cs.json> <witness.json>          Poseidon128<2, 1> over the inputs (1, 2)
//   poseidon_test dump_circuit <r1cs.json> <witness.json> <address> <leaf> <path_0> .. <path_{D-1}>     the membership circuit of depth D
//   poseidon_test tree <width> <depth> <root> <leaf_0> ..         the device tree against a root computed elsewhere              prints PTREE OK
#include "ethsnarks_hip/gadgets.hpp"
#include "ethsnarks_hip/merkle.hpp"

#include <fstream>
#include <iostream>

using namespace ethsnarks;

#define EXPECT(cond) do { if (!(cond)) { std::cerr << "failed: " #cond << std::endl; return 1; } } while (0)

static zk_fr to_fr(const FieldT &v) { const FieldT::bigint b = v.as_bigint(); return zk_fr{b.data[0], b.data[1], b.data[2], b.data[3]}; }
static FieldT from_fr(const zk_fr &v) { FieldT::bigint b; for (int i = 0; i < 4; i++) b.data[i] = v[(size_t)i]; return FieldT(b); }

template <unsigned nIn, unsigned nOut>
static int gadget_agrees(const std::vector<FieldT> &in) {
    ProtoboardT pb;
    const VariableArrayT vars = make_var_array(pb, nIn, "in");
    vars.fill_with_field_elements(pb, in);
    Poseidon128<nIn, nOut> g(pb, vars, "poseidon");
    g.generate_r1cs_witness();
    g.generate_r1cs_constraints();
    EXPECT(pb.num_constraints() == 315 + nOut && pb.num_variables() == nIn + 315 + nOut);
    EXPECT(pb.is_satisfied());
    const std::vector<FieldT> state = poseidon_permutation(in);
    for (unsigned o = 0; o < nOut; o++) EXPECT(pb.val(g.outputs()[o]) == state[o]);
    EXPECT(pb.val(g.result()) == poseidon(in));
    return 0;
}

static int kat() {
    const PoseidonConstants &k = poseidon_params<6, 8, 57>();
    EXPECT(k.C.size() == 65 && k.M.size() == 36);
    EXPECT(k.C[0] == FieldT("14397397413755236225575615486459253198602422701513067526754101844196324375522"));
    EXPECT(k.C[64] == FieldT("10635360132728137321700090133109897687122647659471659996419791842933639708516"));
    EXPECT(k.M[0] == FieldT("19167410339349846567561662441069598364702008768579734801591448511131028229281"));
    EXPECT(k.M[35] == FieldT("20261355950827657195644012399234591122288573679402601053407151083849785332516"));
    const FieldT h12("12242166908188651009877250812424843524687801523336557272219921456462821518061");
    EXPECT(poseidon({FieldT(1), FieldT(2)}) == h12);
    EXPECT(poseidon({FieldT(0), FieldT(0)}) == FieldT("951383894958571821976060584138905353883650994872035011055912076785884444545"));
    ProtoboardT pb;
    const VariableArrayT in = make_var_array(pb, 2, "in");
    pb.val(in[0]) = FieldT(1); pb.val(in[1]) = FieldT(2);
    Poseidon128<2, 1> g(pb, in, "poseidon");
    g.generate_r1cs_witness();
    g.generate_r1cs_constraints();
    EXPECT(pb.num_constraints() == 316 && pb.num_variables() == 2 + 315 + 1);
    EXPECT(pb.is_satisfied() && pb.val(g.result()) == h12 && g.result().index == 3 + 315);
    pb.val(VariableT(100)) += FieldT::one();                     // one S-box variable altered
    EXPECT(!pb.is_satisfied());
    if (gadget_agrees<3, 2>({FieldT(7), FieldT(8), FieldT(9)})) return 1;
    if (gadget_agrees<1, 1>({-FieldT(1)})) return 1;
    if (gadget_agrees<5, 6>({FieldT(0), FieldT(0), FieldT(0), FieldT(0), FieldT(0)})) return 1;
    std::cout << "OK" << std::endl;
    return 0;
}

static int dump(const ProtoboardT &pb, const char *r1cs, const char *witness) {
    std::ofstream(r1cs) << r1cs2json(pb);
    std::ofstream(witness) << witness2json(pb);
    return 0;
}

static int dump_gadget(const char *r1cs, const char *witness) {
    ProtoboardT pb;
    const VariableArrayT in = make_var_array(pb, 2, "in");
    pb.val(in[0]) = FieldT(1); pb.val(in[1]) = FieldT(2);
    Poseidon128<2, 1> g(pb, in, "poseidon");
    g.generate_r1cs_witness();
    g.generate_r1cs_constraints();
    return dump(pb, r1cs, witness);
}

// root (public), address bits, path, leaf; per level a merkle_path_selector, then Poseidon128<2, 1> over (left, right); result * 1 = root
static int dump_circuit(int argc, char **argv) {
    const size_t depth = (size_t)argc - 6;
    const unsigned long address = std::stoul(argv[4]);
    ProtoboardT pb;
    const VariableT root = make_variable(pb, "root");
    pb.set_input_sizes(1);
    const VariableArrayT bits = make_var_array(pb, depth, "address"), path = make_var_array(pb, depth, "path");
    const VariableT leaf = make_variable(pb, FieldT(argv[5]), "leaf");
    bits.fill_with_bits_of_ulong(pb, address);
    for (size_t d = 0; d < depth; d++) pb.val(path[d]) = FieldT(argv[6 + d]);
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
    pb.val(root) = pb.val(item);
    pb.add_r1cs_constraint(ConstraintT(item, 1, root), "result = root");
    EXPECT(pb.is_satisfied() && pb.num_constraints() == 322 * depth + 1);
    return dump(pb, argv[2], argv[3]);
}

static int tree(int argc, char **argv) {
    const uint32_t width = (uint32_t)std::stoul(argv[2]), depth = (uint32_t)std::stoul(argv[3]);
    const zk_fr root = to_fr(FieldT(argv[4]));
    std::vector<zk_fr> leaves;
    for (int i = 5; i < argc; i++) leaves.push_back(to_fr(FieldT(argv[i])));
    const size_t n = leaves.size();
    EXPECT(n >= 2);
    MerkleTreeHIP t(depth, width, MerkleHasher::Poseidon, 2);
    EXPECT(t.empty() && t.width() == width && t.depth() == depth && t.hasher() == MerkleHasher::Poseidon);
    uint32_t d = 0, w = 0; int h = -1;
    EXPECT(zk_mtree_info(t.handle(), &d, &w, &h) == ZK_OK && d == depth && w == width && h == ZK_MTREE_HASH_POSEIDON);
    EXPECT(t.append(leaves[0]) == 0);
    t.extend(std::vector<zk_fr>(leaves.begin() + 1, leaves.end()));
    EXPECT(t.size() == n && t.root() == root && t.node(0, n - 1) == leaves[n - 1]);
    // every proof leads to the root through the host poseidon()
    std::vector<uint64_t> all;
    for (uint64_t i = 0; i < n; i++) all.push_back(i);
    const std::vector<MerkleProofHIP> proofs = t.proofs(all);
    for (uint64_t i = 0; i < n; i++) {
        const MerkleProofHIP &p = proofs[i];
        EXPECT(p.leaf == leaves[i] && p.digits.size() == depth && p.path.size() == (size_t)depth * (width - 1) && p.address.size() == (width == 2 ? depth : 0));
        FieldT item = from_fr(p.leaf);
        for (uint32_t lv = 0; lv < depth; lv++) {
            std::vector<FieldT> args;
            for (uint32_t q = 0; q + 1 < width; q++) args.push_back(from_fr(p.path[(size_t)lv * (width - 1) + q]));
            args.insert(args.begin() + p.digits[lv], item);
            item = poseidon(args);
        }
        EXPECT(to_fr(item) == root);
    }
    // an update and its undoing, the last write winning
    t.update(1, leaves[0]);
    EXPECT(!(t.root() == root));
    t.update_many({1, 0, 1}, {leaves[0], leaves[0], leaves[1]});
    EXPECT(t.root() == root);
    const zk_mtree_layout L = t.membership_layout();
    EXPECT(L.n_iv == 0 && L.root_var == 1 && L.leaf_var == 2 + 2 * depth);
    bool threw = false;
    try { t.update(n, leaves[0]); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);
    threw = false;
    try { MerkleTreeHIP bad(3, 5, MerkleHasher::Poseidon); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);
    threw = false;
    try { MerkleTreeHIP bad(3, 3, MerkleHasher::MiMC); } catch (const mtree_error &e) { threw = e.code == ZK_ERR_ARG; }
    EXPECT(threw);
    MerkleTreeHIP mimc(depth, 2, MerkleHasher::MiMC), plain(depth);        // the MiMC tree through either constructor
    mimc.extend({leaves[0], leaves[1]}); plain.extend({leaves[0], leaves[1]});
    EXPECT(mimc.root() == plain.root() && !(mimc.root() == root));
    std::cout << "PTREE OK" << std::endl;
    return 0;
}

int main(int argc, char **argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "kat") return kat();
        if (mode == "dump_gadget" && argc == 4) return dump_gadget(argv[2], argv[3]);
        if (mode == "dump_circuit" && argc >= 7) return dump_circuit(argc, argv);
        if (mode == "tree" && argc >= 7) return tree(argc, argv);
        std::cerr << "usage: " << argv[0] << " kat | dump_gadget .. | dump_circuit .. | tree .." << std::endl;
        return 2;
    } catch (const std::exception &e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
}
