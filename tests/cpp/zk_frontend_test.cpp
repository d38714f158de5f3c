// tests/cpp/zk_frontend_test.cpp -- zero-knowledge proofs through the C++ adapter (include/ethsnarks_hip/stubs.hpp):
// the MiMC hash circuit of the reference's test_mimc_hash.cpp on a protoboard, a full key made with zk_keygen_full and written as
// the full key stream, then ethsnarks::load_proving_key_full -> ProverContextT -> ethsnarks::prove_zk twice -> stub_verify.
// Compiled by tests/test_zk_emul.py (against the CPU emulation build) and tests/test_zk_gpu.py (against libzkhip.so).
//
//   zk_frontend_test <pk.raw> <vk.json>     prints VERIFIED when both proofs verify and differ (fresh r, s per proof)
#include "ethsnarks_hip/stubs.hpp"
#include "ethsnarks_hip/gadgets.hpp"

#include <fstream>

using namespace ethsnarks;

int main(int argc, char **argv) {
    if (argc != 3) { std::cerr << "usage: " << argv[0] << " <pk.raw> <vk.json>" << std::endl; return 2; }
    ProtoboardT pb;
    const VariableT m_0 = make_variable(pb, FieldT("3703141493535563179657531719960160174296085208671919316200479060314459804651"), "m_0");
    const VariableT m_1 = make_variable(pb, FieldT("134551314051432487569247388144051420116740427803855572138106146683954151557"), "m_1");
    pb.set_input_sizes(2);
    const VariableT iv = make_variable(pb, FieldT("918403109389145570117360101535982733651217667914747213867238065296420114726"), "iv");
    MiMC_e7_hash_gadget the_gadget(pb, iv, {m_0, m_1}, "gadget");
    the_gadget.generate_r1cs_witness();
    the_gadget.generate_r1cs_constraints();
    if (!pb.is_satisfied()) { std::cerr << "circuit not satisfied" << std::endl; return 1; }
    {   // the full key: zk_keygen_full with fresh toxic waste, written as the full stream
        const detail::FlatSystem f(pb.constraint_system);
        const zk_csr a = f.a(), b = f.b(), c = f.c();
        uint64_t toxic[20];
        for (int i = 0; i < 5; i++) { const auto v = FieldT::random_element().as_bigint(); std::memcpy(toxic + 4 * i, v.data, 32); }
        zk_pk *pk = nullptr; zk_vk *vk = nullptr;
        zk_check(zk_keygen_full(&a, &b, &c, f.nC, f.nIn, f.V, toxic, (int)hip_device(), &pk, &vk));
        size_t len = 0;
        zk_vk_to_json(vk, nullptr, 0, &len);
        std::string js(len + 1, '\0');
        zk_check(zk_vk_to_json(vk, &js[0], js.size(), &len));
        js.resize(len);
        std::ofstream(argv[2], std::ios::binary) << js;
        zk_check(zk_pk_save_raw_full(pk, argv[1], ZK_CODEC_ALT_BN128));
        zk_pk_free(pk); zk_vk_free(vk);
    }
    ProvingKeyT pk = load_proving_key_full(argv[1]);
    ProverContextT context(pk);
    context.constraint_system = &pb.constraint_system;
    const std::string p1 = prove_zk(context, pb), p2 = prove_zk(context, pb);
    std::ifstream vf(argv[2], std::ios::binary);
    const std::string vk_json((std::istreambuf_iterator<char>(vf)), std::istreambuf_iterator<char>());
    if (p1 == p2) { std::cerr << "two zero-knowledge proofs of one witness are equal" << std::endl; return 1; }
    if (!stub_verify(vk_json.c_str(), p1.c_str()) || !stub_verify(vk_json.c_str(), p2.c_str())) { std::cerr << "proof rejected" << std::endl; return 1; }
    if (prove(context, pb).find(p1.substr(p1.find("\"input\""))) == std::string::npos) { std::cerr << "public inputs differ" << std::endl; return 1; }
    std::cout << "VERIFIED" << std::endl;
    return 0;
}
