// tests/cpp/verify_batch_test.cpp -- ethsnarks::stub_verify_batch of the C++ adapter (include/ethsnarks_hip/stubs.hpp): the verdicts of a
// batch equal those of stub_verify one by one, a rejected proof does not disturb its neighbours, an unparsable text is `false`.
// Compiled by tests/test_verify_batch_emul.py (against the CPU emulation build) and tests/test_verify_batch_gpu.py (against libzkhip.so).
//
//   verify_batch_test <vk.json> <proof.json> <tampered-proof.json>     prints BATCH OK
#include "ethsnarks_hip/stubs.hpp"

#include <fstream>

using namespace ethsnarks;

static std::string slurp(const char *path) {
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 4) { std::cerr << "usage: " << argv[0] << " <vk.json> <proof.json> <tampered-proof.json>" << std::endl; return 2; }
    const std::string vk = slurp(argv[1]), good = slurp(argv[2]), bad = slurp(argv[3]);
    if (vk.empty() || good.empty() || bad.empty()) { std::cerr << "empty input" << std::endl; return 2; }
    const std::vector<std::string> batch = {good, bad, good, "{ not a proof }", bad, good, good};
    const std::vector<bool> want = {true, false, true, false, false, true, true};
    const std::vector<bool> got = stub_verify_batch(vk.c_str(), batch);
    if (got != want) { std::cerr << "batch verdicts differ from the expected ones" << std::endl; return 1; }
    for (size_t i = 0; i < batch.size(); i++) {
        if (i == 3) continue;                                    // (stub_verify throws on the unparsable text)
        if (stub_verify(vk.c_str(), batch[i].c_str()) != got[i]) { std::cerr << "verdict " << i << " differs from stub_verify" << std::endl; return 1; }
    }
    if (!stub_verify_batch(vk.c_str(), {}).empty()) return 1;
    bool threw = false;
    try { stub_verify_batch("{}", batch); } catch (const zk_error &e) { threw = e.code == ZK_ERR_FORMAT; }
    if (!threw) { std::cerr << "a malformed key must throw ZK_ERR_FORMAT" << std::endl; return 1; }
    std::cout << "BATCH OK" << std::endl;
    return 0;
}
