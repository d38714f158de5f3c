// poseidon.hpp -- the Poseidon permutation of ethsnarks/poseidon/permutation.py (DefaultParams = Poseidon128 of src/gadgets/poseidon.hpp) on the
// device: field Fr, t = 6, 8 full + 57 partial rounds, S-box x^5, ONE round constant per round added to every state element, a 6 x 6 Cauchy
// matrix.  The tree kernels that use it live in merkle.hpp, the entry points (zk_poseidon_*) in merkle.cpp.
//
// Round i (permutation.py:186-189):  ARK  x_j += C_i;  S-box on all six elements (i < 4 or i >= 61) or on x_0 alone;  MIX  x <- M x.  Every
// intermediate state equals the Python one.  One lane per permutation, the state in registers, loose domain (bn254.hpp) with one canon at the end.
// The 65 + 36 constants sit in a device table (Montgomery, canonical) and are read with wave-uniform indices: scalar loads, no per-lane state.
//
// Cost.  An S-box is 3 products; MIX is 36 of the 54 products of a full round and 36 of the 39 of a partial one: 8 x 54 + 57 x 39 = 2 655 products
// per permutation when every matrix entry costs an lmul.  Each MIX output is a six-term dot product with a constant row, so Fr::ldot6 sums the six
// products into the same columns before ONE reduction (6 x 64 + 72 = 456 multiplies instead of 6 x 136 = 816) and takes the row limbs from SGPRs.
// MIX is compiled both ways (template parameter DOT6); POSEIDON_MIX_DOT6 names the form the tree uses (DESIGN 5g has the measurement).
//
// Code size.  The S-box layer and the MIX layer are ROLLED loops over a rotating state (x_0 is worked on, then the state turns by one place):
// one S-box body and one dot-product body per kernel instead of 6 + 6, with 40 register moves per step.  Unrolled, a round is ~45 KB of code,
// most of the instruction cache that the waves of two compute units share.
#pragma once
#include "bn254.hpp"

namespace zk {
namespace poseidon {

constexpr uint32_t T = 6;
constexpr uint32_t ROUNDS_F = 8, ROUNDS_P = 57, ROUNDS = ROUNDS_F + ROUNDS_P;
constexpr uint32_t N_CONSTS = ROUNDS + T * T;                   // the device table: C[65], then M[6][6] row major
constexpr uint32_t BLOCK = 64;
#ifndef ZK_POSEIDON_MIX_LMUL
constexpr bool POSEIDON_MIX_DOT6 = true;
#else
constexpr bool POSEIDON_MIX_DOT6 = false;
#endif

ZK_HD fe pow5(const fe &a) { const fe a2 = Fr::lsqr(a); return Fr::lmul(Fr::lsqr(a2), a); }
ZK_HD void turn(fe (&x)[T]) {
    const fe t = x[0];
#pragma unroll
    for (uint32_t j = 0; j + 1 < T; j++) x[j] = x[j + 1];
    x[T - 1] = t;
}
// one MIX output the plain way: six products, five additions
ZK_HD fe mix_row_lmul(const fe (&x)[T], const fe *__restrict__ row) {
    fe s = Fr::lmul(x[0], row[0]);
#pragma unroll
    for (uint32_t j = 1; j < T; j++) s = Fr::ladd(s, Fr::lmul(x[j], row[j]));
    return s;
}

// the permutation in place; loose in, loose out.  pc: C then M (Montgomery, canonical -- Fr::ldot6 needs a canonical row)
template <bool DOT6>
ZK_HD void permute(const fe *__restrict__ pc, fe (&x)[T]) {
    const fe *__restrict__ M = pc + ROUNDS;
#pragma clang loop unroll(disable)
    for (uint32_t r = 0; r < ROUNDS; r++) {
        const fe c = pc[r];
#pragma unroll
        for (uint32_t j = 0; j < T; j++) x[j] = Fr::ladd(x[j], c);
        const bool full = r < ROUNDS_F / 2 || r >= ROUNDS_F / 2 + ROUNDS_P;
#pragma clang loop unroll(disable)
        for (uint32_t j = 0; j < T; j++) {                      // six turns bring the state back to where it was
            if (j == 0 || full) x[0] = pow5(x[0]);
            turn(x);
        }
        fe y[T];
#pragma unroll
        for (uint32_t j = 0; j < T; j++) y[j] = Fr::zero();
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < T; i++) {                      // y_i enters at the end and has turned to place i after the last step
            const fe o = DOT6 ? Fr::ldot6(x, M + T * i) : mix_row_lmul(x, M + T * i);
            turn(y);
            y[T - 1] = o;
        }
#pragma unroll
        for (uint32_t j = 0; j < T; j++) x[j] = y[j];
    }
}

constexpr uint32_t N_SBOX = ROUNDS_F * T + ROUNDS_P;             // 105 S-boxes, three variables each (FifthPower_gadget: x2, x4, x5)

// permute() with the intermediates of every S-box stored, canonical, in the order the S-boxes run: out[3 s .. 3 s + 2] = x^2, x^4, x^5 of
// S-box s, x the state element after ARK -- the variables Poseidon128's gadget allocates, in its allocation order (merkle.hpp writes a
// membership witness with it).  The same rolled loops; the squarings of pow5 are the stored x^2 and x^4.  Loose in, loose out
template <bool DOT6>
ZK_HD void permute_traced(const fe *__restrict__ pc, fe (&x)[T], fe *__restrict__ out) {
    const fe *__restrict__ M = pc + ROUNDS;
#pragma clang loop unroll(disable)
    for (uint32_t r = 0; r < ROUNDS; r++) {
        const fe c = pc[r];
#pragma unroll
        for (uint32_t j = 0; j < T; j++) x[j] = Fr::ladd(x[j], c);
        const bool full = r < ROUNDS_F / 2 || r >= ROUNDS_F / 2 + ROUNDS_P;
#pragma clang loop unroll(disable)
        for (uint32_t j = 0; j < T; j++) {
            if (j == 0 || full) {
                const fe x2 = Fr::lsqr(x[0]), x4 = Fr::lsqr(x2);
                x[0] = Fr::lmul(x4, x[0]);
                out[0] = Fr::canon(x2); out[1] = Fr::canon(x4); out[2] = Fr::canon(x[0]);
                out += 3;
            }
            turn(x);
        }
        fe y[T];
#pragma unroll
        for (uint32_t j = 0; j < T; j++) y[j] = Fr::zero();
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < T; i++) {
            const fe o = DOT6 ? Fr::ldot6(x, M + T * i) : mix_row_lmul(x, M + T * i);
            turn(y);
            y[T - 1] = o;
        }
#pragma unroll
        for (uint32_t j = 0; j < T; j++) x[j] = y[j];
    }
}

// out[g] = poseidon(in[g n_in .. g n_in + n_in - 1]); canonical in and out (the host has checked the operands against r and 1 <= n_in <= 5)
template <bool DOT6>
__global__ void __launch_bounds__(BLOCK)
k_poseidon_hash(const fe *__restrict__ in, uint32_t n_in, uint32_t n, const fe *__restrict__ pc, fe *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe x[T];
#pragma unroll
    for (uint32_t j = 0; j < T; j++) x[j] = j < n_in ? Fr::to_mont(in[(size_t)g * n_in + j]) : Fr::zero();
    permute<DOT6>(pc, x);
    out[g] = Fr::from_mont(Fr::canon(x[0]));
}

// the "chained" form: n full states of six elements, in place; canonical in and out
template <bool DOT6>
__global__ void __launch_bounds__(BLOCK)
k_poseidon_permute(fe *__restrict__ st, uint32_t n, const fe *__restrict__ pc) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe x[T];
#pragma unroll
    for (uint32_t j = 0; j < T; j++) x[j] = Fr::to_mont(st[(size_t)g * T + j]);
    permute<DOT6>(pc, x);
#pragma unroll
    for (uint32_t j = 0; j < T; j++) st[(size_t)g * T + j] = Fr::from_mont(Fr::canon(x[j]));
}

}  // namespace poseidon
}  // namespace zk
