// blind.hpp -- zero-knowledge blinding of Groth16 proofs on the device (libsnark's r1cs_gg_ppzksnark_prover with the key
// elements of the zok generator, tcc:277-449).  From the per-proof results of the multi-exponentiations and two random
// scalars r, s:
//     A  = alpha1 + At  + r delta1                              (G1)
//     B  = beta2  + Bt  + s delta2                              (G2)
//     B1 = beta1  + B1t + s delta1                              (G1, not part of the proof)
//     C  = Ht + Lt + s A + r B1 - (r s) delta1                  (G1)
// r = s = 0 gives the no-ZK proof (tcc:533-540).
//
//   * fixed-base products (r delta1, s delta1, rs delta1, s delta2): small window-multiple tables of delta built at context
//     creation, T[w][d - 1] = d 2^(c w) delta for signed c-bit digits -- one product is BLIND_W mixed additions, no doublings
//     (the idea the MSM tables use).  The three G1 products need no MSM result: k_zk_blind_fixed computes them at the start of the
//     proof, one quad per product, beside the multi-exponentiations -- off the critical path;
//   * s A + r B1: ONE interleaved (Shamir) chain over the bits of both scalars, table {A, B1, A + B1}: the 254 doublings are shared;
//   * one logical thread per proof, Q = 4 lanes per point operation (Curve::*_q): the chain of a lone proof is latency;
//   * G2 (B) in a kernel of its own, so that the G2 register footprint does not set the occupancy of the G1 work.
// Every step handles the point at infinity (an intermediate A or B1 can be O).  MSM results with S > 1 bucket planes (memory-
// frugal tables, MsmShape::plog) are folded here as MsmWork::finish folds them on the host.
#pragma once
#include <vector>
#include "bn254.hpp"
#include "common.hpp"

namespace zk {

constexpr uint32_t BLIND_C = 6;                          // fixed-base window bits (signed digits)
constexpr uint32_t BLIND_W = 254 / BLIND_C + 1;          // 43 windows (the top one holds bits 252-253 plus a carry: no carry out)
constexpr uint32_t BLIND_D = 1u << (BLIND_C - 1);        // 32 multiples per window
constexpr uint32_t BLIND_ROWS = BLIND_W * BLIND_D;       // table entries of one fixed base
constexpr uint32_t BLIND_Q = 4;                          // lanes per logical thread
constexpr uint32_t BLIND_BLOCK = 64;

// per proof in the buffers of a context: {r, s} canonical (2 fe), {A, C} (2 G1 XYZZ), B (1 G2 XYZZ); on the device also
// {r delta1, s delta1, -(r s) delta1} (3 G1 XYZZ)
constexpr size_t BLIND_RS_BYTES = 2 * sizeof(fe);
constexpr size_t BLIND_G1_BYTES = 2 * sizeof(G1::XYZZ);
constexpr size_t BLIND_G2_BYTES = sizeof(G2::XYZZ);
constexpr size_t BLIND_FIX_BYTES = 3 * sizeof(G1::XYZZ);

// limb i of a scalar by selection, not by a register index the compiler would have to put in scratch memory (0 past the top)
ZK_HD uint32_t blind_limb(const fe &k, uint32_t i) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) v = j == i ? k.l[j] : v;
    return v;
}
ZK_HD uint32_t blind_bit(const fe &k, uint32_t i) { return (blind_limb(k, i >> 5) >> (i & 31)) & 1u; }
ZK_HD uint32_t blind_digit_bits(const fe &k, uint32_t at) {           // BLIND_C bits of a canonical scalar from bit `at`
    const uint32_t li = at >> 5, sh = at & 31;
    const uint64_t v = (((uint64_t)blind_limb(k, li + 1) << 32) | blind_limb(k, li)) >> sh;
    return (uint32_t)v & ((1u << BLIND_C) - 1u);
}

// k T for a canonical scalar k and the table T of a fixed base
template <class C>
ZK_HD typename C::XYZZ blind_fixed(const fe &k, const typename C::Affine *__restrict__ T, uint32_t ql) {
    typename C::XYZZ acc = C::infinity();
    uint32_t carry = 0;
    for (uint32_t w = 0; w < BLIND_W; w++) {
        uint32_t d = blind_digit_bits(k, w * BLIND_C) + carry;
        const bool neg = d > BLIND_D;
        carry = neg ? 1u : 0u;
        if (neg) d = (1u << BLIND_C) - d;
        if (d) {
            typename C::Affine p = T[w * BLIND_D + d - 1];
            if (neg) p = C::neg(p);
            acc = C::template maddQ<BLIND_Q>(acc, p, ql);
        }
    }
    return acc;
}

// MSM result of one proof from its S bucket planes: sum_j 2^(c j) R_j, Horner from the top plane (MsmWork::finish)
template <class C>
ZK_HD typename C::XYZZ blind_fold(const typename C::XYZZ *__restrict__ r, uint32_t S, uint32_t c, uint32_t ql) {
    typename C::XYZZ acc = r[S - 1];
    for (uint32_t j = S - 1; j-- > 0;) {
        for (uint32_t d = 0; d < c; d++) acc = C::template dblQ<BLIND_Q>(acc, ql);
        acc = C::template addQ<BLIND_Q>(acc, r[j], ql);
    }
    return acc;
}

struct BlindG1Args {
    const G1::XYZZ *At, *B1t, *Ht, *Lt;        // MSM results, S planes per proof; Lt == nullptr: the L-query is folded into Ht
    uint32_t S, cA, cB, cH, cL;                 // planes; window bits of the A-, B-, H-, L-query (fold doublings)
    G1::Affine alpha1, beta1;
    const G1::XYZZ *fixed;                      // per proof {r delta1, s delta1, -(r s) delta1} (k_zk_blind_fixed)
    const fe *rs;                               // per proof {r, s}, canonical
    G1::XYZZ *out;                              // per proof {A, C}
    uint32_t k;
};
struct BlindG2Args {
    const G2::XYZZ *Bt;
    uint32_t S, cB;
    G2::Affine beta2;
    const G2::Affine *delta2;
    const fe *rs;
    G2::XYZZ *out;                              // per proof B
    uint32_t k;
};

// (a second unit that wants the fixed-base helpers above only -- verify_gpu.cpp -- defines ZK_BLIND_NO_KERNELS: the kernels below are
// plain definitions and belong to one unit)
#ifndef ZK_BLIND_NO_KERNELS
// r delta1, s delta1, -(r s) delta1 of every proof: quad q = 3 p + j computes product j of proof p
__global__ void __launch_bounds__(BLIND_BLOCK)
k_zk_blind_fixed(const G1::Affine *__restrict__ delta1, const fe *__restrict__ rs_in, G1::XYZZ *__restrict__ out, uint32_t k) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, q = tid / BLIND_Q, ql = tid & (BLIND_Q - 1);
    if (q >= 3 * k) return;
    const uint32_t p = q / 3, j = q - 3 * p;
    const fe r = rs_in[2 * p], s = rs_in[2 * p + 1];
    const fe e = j == 0 ? r : j == 1 ? s : Fr::canon(Fr::mul(Fr::to_mont(r), s));     // (r R) s / R = r s mod r, canonical
    G1::XYZZ P = blind_fixed<G1>(e, delta1, ql);
    if (j == 2) P = G1::neg(P);
    if (ql == 0) out[q] = P;
}

__global__ void __launch_bounds__(BLIND_BLOCK)
k_zk_blind_g1(BlindG1Args a) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, p = tid / BLIND_Q, ql = tid & (BLIND_Q - 1);
    if (p >= a.k) return;                       // (whole quads: the lanes of one proof leave together)
    const fe r = a.rs[2 * p], s = a.rs[2 * p + 1];
    const size_t o = (size_t)p * a.S;
    // A = alpha1 + At + r delta1
    G1::XYZZ A = G1::maddQ<BLIND_Q>(blind_fold<G1>(a.At + o, a.S, a.cA, ql), a.alpha1, ql);
    A = G1::addQ<BLIND_Q>(A, a.fixed[3 * p], ql);
    // B1 = beta1 + B1t + s delta1
    G1::XYZZ B1 = G1::maddQ<BLIND_Q>(blind_fold<G1>(a.B1t + o, a.S, a.cB, ql), a.beta1, ql);
    B1 = G1::addQ<BLIND_Q>(B1, a.fixed[3 * p + 1], ql);
    // Ht + Lt - (r s) delta1
    G1::XYZZ Cc = blind_fold<G1>(a.Ht + o, a.S, a.cH, ql);
    if (a.Lt) Cc = G1::addQ<BLIND_Q>(Cc, blind_fold<G1>(a.Lt + o, a.S, a.cL, ql), ql);
    Cc = G1::addQ<BLIND_Q>(Cc, a.fixed[3 * p + 2], ql);
    // + s A + r B1: one chain of doublings for both scalars
    const G1::XYZZ AB = G1::addQ<BLIND_Q>(A, B1, ql);
    G1::XYZZ acc = G1::infinity();
    for (uint32_t i = 254; i-- > 0;) {
        acc = G1::dblQ<BLIND_Q>(acc, ql);
        const uint32_t sel = blind_bit(s, i) | (blind_bit(r, i) << 1);
        if (sel) {
            G1::XYZZ q = AB;
            if (sel == 1) q = A;
            if (sel == 2) q = B1;
            acc = G1::addQ<BLIND_Q>(acc, q, ql);
        }
    }
    Cc = G1::addQ<BLIND_Q>(Cc, acc, ql);
    if (ql == 0) { a.out[2 * p] = A; a.out[2 * p + 1] = Cc; }
}

__global__ void __launch_bounds__(BLIND_BLOCK)
k_zk_blind_g2(BlindG2Args a) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, p = tid / BLIND_Q, ql = tid & (BLIND_Q - 1);
    if (p >= a.k) return;
    const fe s = a.rs[2 * p + 1];
    G2::XYZZ B = G2::maddQ<BLIND_Q>(blind_fold<G2>(a.Bt + (size_t)p * a.S, a.S, a.cB, ql), a.beta2, ql);
    B = G2::addQ<BLIND_Q>(B, blind_fixed<G2>(s, a.delta2, ql), ql);
    if (ql == 0) a.out[p] = B;
}
#endif  // ZK_BLIND_NO_KERNELS

// host: the fixed-base table of `base`, T[w][d - 1] = d 2^(c w) base (canonical affine)
template <class C>
void blind_table_host(const typename C::Affine &base, std::vector<typename C::Affine> &T) {
    T.resize(BLIND_ROWS);
    typename C::XYZZ row = C::from_affine(base);
    for (uint32_t w = 0; w < BLIND_W; w++) {
        typename C::XYZZ acc = row;
        for (uint32_t d = 0; d < BLIND_D; d++) {
            T[w * BLIND_D + d] = C::to_affine(acc);
            acc = C::add(acc, row);
        }
        for (uint32_t b = 0; b < BLIND_C; b++) row = C::dbl(row);
    }
}

}  // namespace zk
