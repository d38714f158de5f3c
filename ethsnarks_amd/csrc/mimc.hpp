// mimc.hpp -- the MiMC-e7 cipher over Fr and the range check of a canonical value: the parts of the tree's hashing (merkle.hpp) that other
// units use as well (jubjub.hpp: the MiMC variant of EdDSA runs the same cipher over a second constant table).
#pragma once
#include "bn254.hpp"

namespace zk {
namespace merkle {

constexpr uint32_t MIMC_ROUNDS = 91;

// E_k(x) + k of the reference's mimc(): 91 rounds x <- (x + k + c_i)^7, then + k.  Loose in, loose out.
ZK_HD fe mimc_cipher(const fe *__restrict__ rc, const fe &x0, const fe &k) {
    fe x = x0;
    for (uint32_t i = 0; i < MIMC_ROUNDS; i++) {
        const fe t = Fr::ladd(Fr::ladd(x, k), rc[i]);
        const fe t2 = Fr::lsqr(t);
        const fe t4 = Fr::lsqr(t2);
        const fe t6 = Fr::lmul(t4, t2);
        x = Fr::lmul(t6, t);
    }
    return Fr::ladd(x, k);
}
ZK_HD bool fr_lt_modulus(const fe &a) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.l[i] - FrParams::p(i) - br; br = (t >> 32) & 1; }
    return br != 0;
}

}  // namespace merkle
}  // namespace zk
