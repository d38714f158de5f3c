// ethsnarks_hip/gadgets.hpp -- the two self-contained ethsnarks circuits the measurement configs name
// (BASELINE configs 1 and 4), written against the stand-alone front end of circuit.hpp:
//
//   MiMCe7_round, MiMC_gadget<RoundT>, MiMC_e7_gadget        src/gadgets/mimc.hpp:115-318
//   MiyaguchiPreneel_OWF<CipherT>, MiMC_e7_hash_gadget       src/gadgets/onewayfunction.hpp:67-127, mimc.hpp:321-346
//   merkle_path_selector                                     src/gadgets/merkle_tree.hpp:35-63, merkle_tree.cpp:11-72
//   markle_path_compute<HashT>, merkle_path_authenticator    src/gadgets/merkle_tree.hpp:71-191  (the reference spells "markle")
//   merkle_tree_IVs                                          src/gadgets/merkle_tree.cpp:75-113 (= ethsnarks/merkletree.py:36-44)
//   mimc(), mimc_hash()                                      src/gadgets/mimc.hpp:352-393 (native evaluation through a protoboard)
//   FifthPower_gadget, Poseidon_gadget_T, Poseidon128, poseidon()    src/gadgets/poseidon.hpp, ethsnarks/poseidon/permutation.py
//
// Same class names, constructor arguments, variable allocation order and constraint order as the reference, so a
// circuit built here has the reference's shape (depth-29 authenticator: 21 345 constraints) and the reference's
// known answers hold (tests/cpp/frontend_test.cpp).  The hash primitives the constants need -- Keccak-256 (original
// 0x01 padding, the reference's SHA3IUF dependency) and SHA-256 (merkletree.py's IV chain) -- are included so
// nothing outside this header is required.  Not compiled when libsnark is present: the reference's own gadget
// headers are the ones to use then.
#pragma once
#include "circuit.hpp"

#include <cassert>
#include <mutex>

namespace ethsnarks {

// ------------------------------------------------------------------------------------------ Keccak-256 / SHA-256
namespace hashes {
inline uint64_t rotl64(uint64_t v, unsigned n) { n &= 63; return n ? (v << n) | (v >> (64 - n)) : v; }
inline void keccak_f1600(uint64_t s[25]) {
    static const uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808AULL, 0x8000000080008000ULL, 0x000000000000808BULL, 0x0000000080000001ULL,
        0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008AULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000AULL,
        0x000000008000808BULL, 0x800000000000008BULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
        0x000000000000800AULL, 0x800000008000000AULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    static const unsigned ROT[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};   // [x][y]
    for (int round = 0; round < 24; round++) {
        uint64_t C[5], B[25];
        for (int x = 0; x < 5; x++) C[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
        for (int x = 0; x < 5; x++) { const uint64_t D = C[(x + 4) % 5] ^ rotl64(C[(x + 1) % 5], 1); for (int y = 0; y < 5; y++) s[x + 5 * y] ^= D; }
        for (int x = 0; x < 5; x++) for (int y = 0; y < 5; y++) B[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(s[x + 5 * y], ROT[x][y]);
        for (int x = 0; x < 5; x++) for (int y = 0; y < 5; y++) s[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
        s[0] ^= RC[round];
    }
}
inline void keccak256(const uint8_t *data, size_t len, uint8_t out[32]) {
    const size_t rate = 136;
    std::vector<uint8_t> p(data, data + len);
    p.push_back(0x01);
    while (p.size() % rate) p.push_back(0);
    p.back() |= 0x80;
    uint64_t s[25] = {0};
    for (size_t off = 0; off < p.size(); off += rate) {
        for (size_t i = 0; i < rate / 8; i++) { uint64_t v = 0; for (int k = 7; k >= 0; k--) v = (v << 8) | p[off + 8 * i + (size_t)k]; s[i] ^= v; }
        keccak_f1600(s);
    }
    for (int i = 0; i < 4; i++) for (int k = 0; k < 8; k++) out[8 * i + k] = (uint8_t)(s[i] >> (8 * k));
}

struct sha256 {                                              // streaming, so a running digest can be read after every update
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    std::vector<uint8_t> buf;
    uint64_t total = 0;
    static uint32_t rotr(uint32_t v, unsigned n) { return (v >> n) | (v << (32 - n)); }
    static void block(uint32_t h[8], const uint8_t *b) {
        static const uint32_t K[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
            0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
            0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
            0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
            0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
            0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        uint32_t w[64];
        for (int i = 0; i < 16; i++) w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
        for (int i = 16; i < 64; i++) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], bb = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & bb) ^ (a & c) ^ (bb & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = bb; bb = a; a = t1 + t2;
        }
        h[0] += a; h[1] += bb; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t *d, size_t n) {
        total += n;
        buf.insert(buf.end(), d, d + n);
        size_t off = 0;
        for (; off + 64 <= buf.size(); off += 64) block(h, buf.data() + off);
        buf.erase(buf.begin(), buf.begin() + (long)off);
    }
    void digest(uint8_t out[32]) const {                     // non-destructive: the stream can continue afterwards
        uint32_t hc[8]; memcpy(hc, h, sizeof(hc));
        std::vector<uint8_t> p(buf);
        p.push_back(0x80);
        while (p.size() % 64 != 56) p.push_back(0);
        const uint64_t bits = total * 8;
        for (int k = 7; k >= 0; k--) p.push_back((uint8_t)(bits >> (8 * k)));
        for (size_t off = 0; off < p.size(); off += 64) block(hc, p.data() + off);
        for (int i = 0; i < 8; i++) for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(hc[i] >> (24 - 8 * k));
    }
};

// BLAKE2b (RFC 7693), unkeyed, digest of 1 .. 64 bytes: the chain behind the Poseidon constants
inline uint64_t rotr64(uint64_t v, unsigned n) { return (v >> n) | (v << (64 - n)); }
inline void blake2b_compress(uint64_t h[8], const uint8_t block[128], uint64_t t, bool last) {
    static const uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                   0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    static const uint8_t SIGMA[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; i++) { m[i] = 0; for (int k = 7; k >= 0; k--) m[i] = (m[i] << 8) | block[8 * i + k]; }
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= t;                                              // (the high counter word stays 0: inputs are far below 2^64 bytes)
    if (last) v[14] = ~v[14];
    for (int r = 0; r < 12; r++) {
        const uint8_t *s = SIGMA[r % 10];
        auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
            v[a] = v[a] + v[b] + x; v[d] = rotr64(v[d] ^ v[a], 32); v[c] = v[c] + v[d]; v[b] = rotr64(v[b] ^ v[c], 24);
            v[a] = v[a] + v[b] + y; v[d] = rotr64(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr64(v[b] ^ v[c], 63);
        };
        G(0, 4, 8, 12, m[s[0]], m[s[1]]); G(1, 5, 9, 13, m[s[2]], m[s[3]]); G(2, 6, 10, 14, m[s[4]], m[s[5]]); G(3, 7, 11, 15, m[s[6]], m[s[7]]);
        G(0, 5, 10, 15, m[s[8]], m[s[9]]); G(1, 6, 11, 12, m[s[10]], m[s[11]]); G(2, 7, 8, 13, m[s[12]], m[s[13]]); G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}
inline void blake2b(const uint8_t *data, size_t len, uint8_t *out, size_t outlen = 32) {
    static const uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                   0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    uint64_t h[8];
    for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= 0x01010000ULL ^ (uint64_t)outlen;                // parameter block: digest length, no key, fanout = depth = 1
    size_t off = 0;
    uint8_t block[128];
    while (len - off > 128) { memcpy(block, data + off, 128); off += 128; blake2b_compress(h, block, off, false); }
    memset(block, 0, 128);
    if (len > off) memcpy(block, data + off, len - off);
    blake2b_compress(h, block, len, true);                   // the last block (also the only one of an empty message), zero padded
    for (size_t i = 0; i < outlen; i++) out[i] = (uint8_t)(h[i / 8] >> (8 * (i % 8)));
}
}  // namespace hashes

// ------------------------------------------------------------------------------------------ MiMC
#define MIMC_SEED "mimc"

// one round: t = x + k + C;  a = t^2, b = t^4, c = t^6, d = t^7 (+ k in the last round)
class MiMCe7_round : public GadgetT {
public:
    static constexpr size_t N_ROUNDS = 91;
    const VariableT x, k;
    const FieldT C;
    const bool add_k_to_result;
    const VariableT a, b, c, d;

    MiMCe7_round(ProtoboardT &in_pb, const VariableT in_x, const VariableT in_k, const FieldT &in_C, const bool in_add_k_to_result,
                 const std::string &annotation_prefix)
        : GadgetT(in_pb, annotation_prefix), x(in_x), k(in_k), C(in_C), add_k_to_result(in_add_k_to_result),
          a(make_variable(in_pb, FMT(annotation_prefix, ".a"))), b(make_variable(in_pb, FMT(annotation_prefix, ".b"))),
          c(make_variable(in_pb, FMT(annotation_prefix, ".c"))), d(make_variable(in_pb, FMT(annotation_prefix, ".d"))) {}

    const VariableT &result() const { return d; }

    void generate_r1cs_constraints() {
        const LinearCombinationT t = x + k + C;
        pb.add_r1cs_constraint(ConstraintT(t, t, a), ".a = t^2");
        pb.add_r1cs_constraint(ConstraintT(a, a, b), ".b = t^4");
        pb.add_r1cs_constraint(ConstraintT(a, b, c), ".c = t^6");
        if (add_k_to_result) pb.add_r1cs_constraint(ConstraintT(t, c, d - k), ".d = t^7 + k");
        else pb.add_r1cs_constraint(ConstraintT(t, c, d), ".d = t^7");
    }
    void generate_r1cs_witness() const {
        const FieldT vk = pb.val(k), t = pb.val(x) + vk + C;
        const FieldT va = t * t, vb = va * va, vc = va * vb;
        pb.val(a) = va; pb.val(b) = vb; pb.val(c) = vc;
        pb.val(d) = vc * t + (add_k_to_result ? vk : FieldT::zero());
    }
};

template <typename RoundT>
class MiMC_gadget : public GadgetT {
public:
    std::vector<RoundT> m_rounds;
    const VariableT k;

    MiMC_gadget(ProtoboardT &in_pb, const VariableT in_x, const VariableT in_k, const std::vector<FieldT> &in_round_constants, const std::string &annotation_prefix)
        : GadgetT(in_pb, annotation_prefix), k(in_k) { setup(in_x, in_k, in_round_constants); }
    MiMC_gadget(ProtoboardT &in_pb, const VariableT in_x, const VariableT in_k, const std::string &annotation_prefix)
        : GadgetT(in_pb, annotation_prefix), k(in_k) { setup(in_x, in_k, static_constants()); }

    const VariableT &result() const { return m_rounds.back().result(); }
    void generate_r1cs_constraints() { for (auto &r : m_rounds) r.generate_r1cs_constraints(); }
    void generate_r1cs_witness() const { for (auto &r : m_rounds) r.generate_r1cs_witness(); }

    // C_0 = keccak256(keccak256(seed)), C_{i+1} = keccak256(C_i), read big-endian and reduced into the field
    static void constants_fill(std::vector<FieldT> &round_constants, const char *seed = MIMC_SEED) {
        uint8_t digest[32];
        hashes::keccak256(reinterpret_cast<const uint8_t *>(seed), strlen(seed), digest);
        round_constants.reserve(RoundT::N_ROUNDS);
        for (size_t i = 0; i < RoundT::N_ROUNDS; i++) {
            uint8_t next[32];
            hashes::keccak256(digest, 32, next);
            memcpy(digest, next, 32);
            round_constants.push_back(FieldT::from_bytes_be(digest));
        }
    }
    static const std::vector<FieldT> constants(const char *seed = MIMC_SEED) { std::vector<FieldT> c; constants_fill(c, seed); return c; }
    static const std::vector<FieldT> &static_constants() {
        static std::vector<FieldT> cached;
        static std::once_flag once;
        std::call_once(once, []() { constants_fill(cached); });
        return cached;
    }

private:
    void setup(const VariableT in_x, const VariableT in_k, const std::vector<FieldT> &rc) {
        m_rounds.reserve(rc.size());
        for (size_t i = 0; i < rc.size(); i++) {
            const VariableT round_x = i == 0 ? in_x : m_rounds.back().result();
            m_rounds.emplace_back(pb, round_x, in_k, rc[i], i + 1 == rc.size(), FMT(annotation_prefix, ".round[%zu]", i));
        }
    }
};
using MiMC_e7_gadget = MiMC_gadget<MiMCe7_round>;

// Miyaguchi-Preneel one-way function: k_{i+1} = k_i + E_{k_i}(m_i) + m_i
template <class CipherT>
class MiyaguchiPreneel_OWF : public GadgetT {
public:
    std::vector<CipherT> m_ciphers;
    const std::vector<VariableT> m_messages;
    const VariableArrayT m_outputs;
    const VariableT m_IV;

    MiyaguchiPreneel_OWF(ProtoboardT &in_pb, const VariableT in_IV, const std::vector<VariableT> &in_messages, const std::string &in_annotation_prefix)
        : GadgetT(in_pb, in_annotation_prefix), m_messages(in_messages),
          m_outputs(make_var_array(in_pb, in_messages.size(), FMT(in_annotation_prefix, ".outputs"))), m_IV(in_IV) {
        m_ciphers.reserve(in_messages.size());
        for (size_t i = 0; i < in_messages.size(); i++)
            m_ciphers.emplace_back(in_pb, in_messages[i], i == 0 ? in_IV : m_outputs[i - 1], FMT(in_annotation_prefix, ".cipher[%zu]", i));
    }
    const VariableT &result() const { return m_outputs[m_outputs.size() - 1]; }
    void generate_r1cs_constraints() {
        for (size_t i = 0; i < m_ciphers.size(); i++) {
            m_ciphers[i].generate_r1cs_constraints();
            const VariableT round_key = i == 0 ? m_IV : m_outputs[i - 1];
            pb.add_r1cs_constraint(ConstraintT(round_key + m_ciphers[i].result() + m_messages[i], 1, m_outputs[i]), ".out = k + E_k(m_i) + m_i");
        }
    }
    void generate_r1cs_witness() const {
        for (size_t i = 0; i < m_ciphers.size(); i++) {
            m_ciphers[i].generate_r1cs_witness();
            const FieldT round_key = i == 0 ? pb.val(m_IV) : pb.val(m_outputs[i - 1]);
            pb.val(m_outputs[i]) = round_key + pb.val(m_ciphers[i].result()) + pb.val(m_messages[i]);
        }
    }
};
template <typename G> using MiMC_hash_MiyaguchiPreneel_gadget = MiyaguchiPreneel_OWF<G>;
using MiMC_e7_hash_gadget = MiMC_hash_MiyaguchiPreneel_gadget<MiMC_e7_gadget>;

// native evaluation, done the way the reference does it: through a scratch protoboard
inline const FieldT mimc(const std::vector<FieldT> &round_constants, const FieldT &x, const FieldT &k) {
    ProtoboardT pb;
    const VariableT vx = make_variable(pb, x, "x"), vk = make_variable(pb, k, "k");
    MiMC_e7_gadget g(pb, vx, vk, round_constants, "mimc");
    g.generate_r1cs_witness();
    return pb.val(g.result());
}
inline const FieldT mimc(const FieldT &x, const FieldT &k) { return mimc(MiMC_e7_gadget::static_constants(), x, k); }
inline const FieldT mimc_hash(const std::vector<FieldT> &m, const FieldT &iv = FieldT::zero()) {
    ProtoboardT pb;
    const VariableT viv = make_variable(pb, iv, "iv");
    std::vector<VariableT> vars;
    for (const auto &v : m) vars.push_back(make_variable(pb, v, "m"));
    MiMC_e7_hash_gadget g(pb, viv, vars, "mimc_hash");
    g.generate_r1cs_witness();
    return pb.val(g.result());
}

// ------------------------------------------------------------------------------------------ Poseidon
// Poseidon128 = the permutation of ethsnarks/poseidon/permutation.py (DefaultParams: t = 6, 8 full + 57 partial rounds, x^5, one constant per
// round, a Cauchy matrix) as a gadget with the reference's names (src/gadgets/poseidon.hpp): FifthPower_gadget, Poseidon_gadget_T, Poseidon128.
// Variables: x2, x4, x5 per S-box in round order (six S-boxes in a full round, one in a partial round), then the output variables; constraints:
// three per S-box in that order, then one  lc * 1 = out  per output -- what the reference's master gadget lays down and what
// ethsnarks_amd/gadgets.py PoseidonGadget builds.  An element that passes a round without an S-box stays a linear combination; its round
// constant is collected into the ONE term of every output of the round.
struct PoseidonConstants {
    std::vector<FieldT> C;                                   // one per round
    std::vector<FieldT> M;                                   // t x t, row major
};
// blake2b-256 chain: the seed is hashed, then the raw digest again; every digest little-endian, reduced mod r (the chain runs unreduced)
inline void poseidon_constants_fill(const std::string &seed, unsigned n_constants, std::vector<FieldT> &result) {
    uint8_t digest[32], next[32], be[32];
    hashes::blake2b(reinterpret_cast<const uint8_t *>(seed.data()), seed.size(), digest);
    result.reserve(result.size() + n_constants);
    for (unsigned i = 0; i < n_constants; i++) {
        for (int k = 0; k < 32; k++) be[k] = digest[31 - k];
        result.push_back(FieldT::from_bytes_be(be));
        hashes::blake2b(digest, 32, next);
        memcpy(digest, next, 32);
    }
}
inline const std::vector<FieldT> poseidon_constants(const std::string &seed, unsigned n_constants) { std::vector<FieldT> r; poseidon_constants_fill(seed, n_constants, r); return r; }
inline void poseidon_matrix_fill(const std::string &seed, unsigned t, std::vector<FieldT> &result) {
    const std::vector<FieldT> c = poseidon_constants(seed, 2 * t);
    result.reserve(result.size() + t * t);
    for (unsigned i = 0; i < t; i++) for (unsigned j = 0; j < t; j++) result.push_back((c[i] - c[t + j]).inverse());
}
inline const std::vector<FieldT> poseidon_matrix(const std::string &seed, unsigned t) { std::vector<FieldT> r; poseidon_matrix_fill(seed, t, r); return r; }
template <unsigned param_t, unsigned param_F, unsigned param_P>
const PoseidonConstants &poseidon_params() {
    static PoseidonConstants constants;
    static std::once_flag once;
    std::call_once(once, []() {
        poseidon_constants_fill("poseidon_constants", param_F + param_P, constants.C);
        poseidon_matrix_fill("poseidon_matrix_0000", param_t, constants.M);
    });
    return constants;
}

// x2 = x x, x4 = x2 x2, x5 = x x4 for a linear combination x
class FifthPower_gadget : public GadgetT {
public:
    const VariableT x2, x4, x5;
    FifthPower_gadget(ProtoboardT &in_pb, const std::string &annotation_prefix)
        : GadgetT(in_pb, annotation_prefix), x2(make_variable(in_pb, FMT(annotation_prefix, ".x2"))), x4(make_variable(in_pb, FMT(annotation_prefix, ".x4"))),
          x5(make_variable(in_pb, FMT(annotation_prefix, ".x5"))) {}
    const VariableT &result() const { return x5; }
    void generate_r1cs_constraints(const LinearCombinationT &x) const {
        pb.add_r1cs_constraint(ConstraintT(x, x, x2), ".x^2 = x * x");
        pb.add_r1cs_constraint(ConstraintT(x2, x2, x4), ".x^4 = x2 * x2");
        pb.add_r1cs_constraint(ConstraintT(x, x4, x5), ".x^5 = x * x4");
    }
    void generate_r1cs_witness(const FieldT &val_x) const {
        const FieldT v2 = val_x * val_x, v4 = v2 * v2;
        pb.val(x2) = v2; pb.val(x4) = v4; pb.val(x5) = v4 * val_x;
    }
};

template <unsigned param_t, unsigned param_c, unsigned param_F, unsigned param_P, unsigned nInputs, unsigned nOutputs, bool constrainOutputs = true>
class Poseidon_gadget_T : public GadgetT {
    static_assert(nInputs > 0 && nInputs < param_t && nOutputs > 0 && nOutputs <= param_t && param_F % 2 == 0, "Poseidon: 0 < nInputs < t, 0 < nOutputs <= t");
    // one round: S-boxes on the first n_sbox elements of `state` (+ C_i), n_in of which exist; the outputs are rows of M over the results
    struct Round {
        FieldT C_i;
        unsigned n_in;
        std::vector<LinearCombinationT> state;
        std::vector<FifthPower_gadget> sboxes;
        std::vector<LinearCombinationT> outputs;
    };
    std::vector<Round> rounds;

public:
    const PoseidonConstants &constants;
    VariableArrayT _output_vars;
    static constexpr unsigned partial_begin = param_F / 2, partial_end = partial_begin + param_P, total_rounds = param_F + param_P;

    Poseidon_gadget_T(ProtoboardT &in_pb, const VariableArrayT &in_inputs, const std::string &annotation_prefix)
        : GadgetT(in_pb, annotation_prefix), constants(poseidon_params<param_t, param_F, param_P>()) {
        if (in_inputs.size() != nInputs) throw std::invalid_argument("Poseidon: the input array does not have nInputs variables");
        std::vector<LinearCombinationT> state(in_inputs.begin(), in_inputs.end());
        rounds.reserve(total_rounds);
        for (unsigned i = 0; i < total_rounds; i++) {
            const unsigned n_sbox = i < partial_begin || i >= partial_end ? param_t : param_c;
            const unsigned n_out = i + 1 == total_rounds ? nOutputs : param_t;
            Round r;
            r.C_i = constants.C[i]; r.n_in = i == 0 ? nInputs : param_t; r.state = state;
            r.sboxes.reserve(n_sbox);
            for (unsigned h = 0; h < n_sbox; h++) r.sboxes.emplace_back(in_pb, FMT(annotation_prefix, ".round[%u].sbox[%u]", i, h));
            for (unsigned o = 0; o < n_out; o++) {
                const FieldT *row = &constants.M[o * param_t];
                LinearCombinationT lc;
                FieldT constant_term;
                for (unsigned j = n_sbox; j < param_t; j++) constant_term += r.C_i * row[j];
                lc.add_term(0, constant_term);
                for (unsigned h = 0; h < n_sbox; h++) lc.add_term(r.sboxes[h].result().index, row[h]);
                for (unsigned k = n_sbox; k < r.n_in; k++) lc = lc + r.state[k] * row[k];
                r.outputs.push_back(lc);
            }
            state = r.outputs;
            rounds.push_back(std::move(r));
        }
        if (constrainOutputs) _output_vars = make_var_array(in_pb, nOutputs, FMT(annotation_prefix, ".output"));
    }
    const std::vector<LinearCombinationT> &output_lcs() const { return rounds.back().outputs; }
    const VariableArrayT &outputs() const { return _output_vars; }
    const VariableT &result() const { return _output_vars.at(0); }

    void generate_r1cs_constraints() const {
        for (const Round &r : rounds)
            for (unsigned h = 0; h < r.sboxes.size(); h++)
                r.sboxes[h].generate_r1cs_constraints(h < r.n_in ? r.state[h] + LinearCombinationT(r.C_i) : LinearCombinationT(r.C_i));
        if (constrainOutputs)
            for (unsigned o = 0; o < nOutputs; o++) pb.add_r1cs_constraint(ConstraintT(rounds.back().outputs[o], 1, _output_vars[o]), ".output = last_round.output");
    }
    void generate_r1cs_witness() const {
        for (const Round &r : rounds)
            for (unsigned h = 0; h < r.sboxes.size(); h++) r.sboxes[h].generate_r1cs_witness(h < r.n_in ? r.C_i + pb.lc_val(r.state[h]) : r.C_i);
        if (constrainOutputs)
            for (unsigned o = 0; o < nOutputs; o++) pb.val(_output_vars[o]) = pb.lc_val(rounds.back().outputs[o]);
    }
};
template <unsigned nInputs, unsigned nOutputs, bool constrainOutputs = true>
using Poseidon128 = Poseidon_gadget_T<6, 1, 8, 57, nInputs, nOutputs, constrainOutputs>;

// native evaluation (permutation.py:150-196), plain field arithmetic: the state after the permutation of (inputs, 0, ..)
inline std::vector<FieldT> poseidon_permutation(const std::vector<FieldT> &inputs) {
    constexpr unsigned t = 6, F = 8, P = 57;
    if (inputs.empty() || inputs.size() > t) throw std::invalid_argument("poseidon: 1 .. 6 state elements");
    const PoseidonConstants &k = poseidon_params<t, F, P>();
    std::vector<FieldT> state(inputs);
    state.resize(t);
    for (unsigned i = 0; i < F + P; i++) {
        for (auto &v : state) v += k.C[i];
        const unsigned n_sbox = i < F / 2 || i >= F / 2 + P ? t : 1;
        for (unsigned j = 0; j < n_sbox; j++) { const FieldT v2 = state[j] * state[j]; state[j] = v2 * v2 * state[j]; }
        std::vector<FieldT> next(t);
        for (unsigned r = 0; r < t; r++) for (unsigned j = 0; j < t; j++) next[r] += k.M[r * t + j] * state[j];
        state = next;
    }
    return state;
}
inline const FieldT poseidon(const std::vector<FieldT> &inputs) {
    if (inputs.size() >= 6) throw std::invalid_argument("poseidon: a hash takes 1 .. 5 inputs");
    return poseidon_permutation(inputs)[0];
}

// ------------------------------------------------------------------------------------------ Merkle path
// left = (1 - is_right) * input + is_right * pathvar;  right = is_right * input + (1 - is_right) * pathvar
class merkle_path_selector : public GadgetT {
public:
    const VariableT m_input, m_pathvar, m_is_right;
    VariableT m_left_a, m_left_b, m_left, m_right_a, m_right_b, m_right;

    merkle_path_selector(ProtoboardT &in_pb, const VariableT &in_input, const VariableT &in_pathvar, const VariableT &in_is_right, const std::string &in_annotation_prefix)
        : GadgetT(in_pb, in_annotation_prefix), m_input(in_input), m_pathvar(in_pathvar), m_is_right(in_is_right) {
        m_left_a.allocate(in_pb, FMT(annotation_prefix, ".left_a"));
        m_left_b.allocate(in_pb, FMT(annotation_prefix, ".left_b"));
        m_left.allocate(in_pb, FMT(annotation_prefix, ".left"));
        m_right_a.allocate(in_pb, FMT(annotation_prefix, ".right_a"));
        m_right_b.allocate(in_pb, FMT(annotation_prefix, ".right_b"));
        m_right.allocate(in_pb, FMT(annotation_prefix, ".right"));
    }
    void generate_r1cs_constraints() {
        pb.add_r1cs_constraint(ConstraintT(1 - m_is_right, m_input, m_left_a), "(1-is_right) * input = left_a");
        pb.add_r1cs_constraint(ConstraintT(m_is_right, m_pathvar, m_left_b), "is_right * pathvar = left_b");
        pb.add_r1cs_constraint(ConstraintT(m_left_a + m_left_b, 1, m_left), "left_a + left_b = left");
        pb.add_r1cs_constraint(ConstraintT(m_is_right, m_input, m_right_a), "is_right * input = right_a");
        pb.add_r1cs_constraint(ConstraintT(1 - m_is_right, m_pathvar, m_right_b), "(1-is_right) * pathvar = right_b");
        pb.add_r1cs_constraint(ConstraintT(m_right_a + m_right_b, 1, m_right), "right_a + right_b = right");
    }
    void generate_r1cs_witness() const {
        const FieldT r = pb.val(m_is_right), nr = FieldT::one() - r;
        pb.val(m_left_a) = nr * pb.val(m_input);
        pb.val(m_left_b) = r * pb.val(m_pathvar);
        pb.val(m_left) = pb.val(m_left_a) + pb.val(m_left_b);
        pb.val(m_right_a) = r * pb.val(m_input);
        pb.val(m_right_b) = nr * pb.val(m_pathvar);
        pb.val(m_right) = pb.val(m_right_a) + pb.val(m_right_b);
    }
    const VariableT &left() const { return m_left; }
    const VariableT &right() const { return m_right; }
};

// per-level IVs: IV_i = sha256("MerkleTree-" || le16(0) || ... || "MerkleTree-" || le16(i)) mod r (running digest)
inline std::vector<FieldT> merkle_tree_IV_values(size_t depth = 29) {
    std::vector<FieldT> out;
    hashes::sha256 h;
    for (size_t i = 0; i < depth; i++) {
        uint8_t msg[13] = {'M', 'e', 'r', 'k', 'l', 'e', 'T', 'r', 'e', 'e', '-', (uint8_t)(i & 0xff), (uint8_t)(i >> 8)};
        h.update(msg, sizeof(msg));
        uint8_t d[32];
        h.digest(d);
        out.push_back(FieldT::from_bytes_be(d));
    }
    return out;
}
inline const VariableArrayT merkle_tree_IVs(ProtoboardT &in_pb) {
    const VariableArrayT x = make_var_array(in_pb, 29, "IVs");
    x.fill_with_field_elements(in_pb, merkle_tree_IV_values(29));
    return x;
}

template <typename HashT>
class markle_path_compute : public GadgetT {
public:
    const size_t m_depth;
    const VariableArrayT m_address_bits;
    const VariableT m_leaf;
    const VariableArrayT m_path;
    std::vector<merkle_path_selector> m_selectors;
    std::vector<HashT> m_hashers;

    markle_path_compute(ProtoboardT &in_pb, const size_t in_depth, const VariableArrayT &in_address_bits, const VariableArrayT &in_IVs,
                        const VariableT in_leaf, const VariableArrayT &in_path, const std::string &in_annotation_prefix)
        : GadgetT(in_pb, in_annotation_prefix), m_depth(in_depth), m_address_bits(in_address_bits), m_leaf(in_leaf), m_path(in_path) {
        if (in_depth == 0 || in_address_bits.size() != in_depth || in_IVs.size() < in_depth || in_path.size() < in_depth)
            throw std::invalid_argument("markle_path_compute: depth, address bits, IVs and path do not agree");
        m_selectors.reserve(in_depth); m_hashers.reserve(in_depth);
        for (size_t i = 0; i < m_depth; i++) {
            const VariableT below = i == 0 ? in_leaf : m_hashers[i - 1].result();
            m_selectors.emplace_back(in_pb, below, in_path[i], in_address_bits[i], FMT(annotation_prefix, ".selector[%zu]", i));
            m_hashers.emplace_back(in_pb, in_IVs[i], std::vector<VariableT>{m_selectors[i].left(), m_selectors[i].right()}, FMT(annotation_prefix, ".hasher[%zu]", i));
        }
    }
    const VariableT result() const { return m_hashers.back().result(); }
    void generate_r1cs_constraints() {
        for (size_t i = 0; i < m_hashers.size(); i++) { m_selectors[i].generate_r1cs_constraints(); m_hashers[i].generate_r1cs_constraints(); }
    }
    void generate_r1cs_witness() const {
        for (size_t i = 0; i < m_hashers.size(); i++) { m_selectors[i].generate_r1cs_witness(); m_hashers[i].generate_r1cs_witness(); }
    }
};

template <typename HashT>
class merkle_path_authenticator : public markle_path_compute<HashT> {
public:
    const VariableT m_expected_root;
    merkle_path_authenticator(ProtoboardT &in_pb, const size_t in_depth, const VariableArrayT in_address_bits, const VariableArrayT in_IVs,
                              const VariableT in_leaf, const VariableT in_expected_root, const VariableArrayT in_path, const std::string &in_annotation_prefix)
        : markle_path_compute<HashT>(in_pb, in_depth, in_address_bits, in_IVs, in_leaf, in_path, in_annotation_prefix), m_expected_root(in_expected_root) {}
    bool is_valid() const { return this->pb.val(this->result()) == this->pb.val(m_expected_root); }
    void generate_r1cs_constraints() {
        markle_path_compute<HashT>::generate_r1cs_constraints();
        this->pb.add_r1cs_constraint(ConstraintT(this->result(), 1, m_expected_root), FMT(this->annotation_prefix, ".expected_root authenticator"));
    }
};

}  // namespace ethsnarks
