// hlagrange.hpp -- the H-query in coset-Lagrange bases: per KEY AND CIRCUIT, once, at context creation.
//
// h = (q - C) / Z(g) with q = A B mod (x^m - g^m): q is given by its values p_j = A(g w^j) B(g w^j) on the coset, C by its values
// c_j = <C_j, witness> on the domain.  Both maps "values -> coefficients" are linear, so they are applied to the H-query BASES here
// instead of to the scalars of every proof:
//     Ht = sum_j p_j Q_j - sum_j c_j Lambda_j
//     Lambda_j = 1 / (m Z(g)) sum_{i < m-1} w^(-ij) H_i              (inverse group DFT of (H_0 .. H_{m-2}, O))
//     Q_j      = 1 / (m Z(g)) sum_{i < m-1} g^(-i) w^(-ij) H_i       (the same DFT of g^(-i) H_i)
// and the second sum is folded into the L-query, whose scalars are the witness:  sum_j c_j Lambda_j = sum_v w_v K_v,
//     K_v = sum_j C[j][v] Lambda_j,       Ht + Lt = sum_j p_j Q_j + sum_{v <= V} w_v (L_v - K_v)       (L_v = O for v <= nIn).
// The proof then needs four transforms instead of six (zkhip.cpp enqueue_compute_h4), and the same unique group element comes out.
//
// Kernels: a radix-2 decimation-in-frequency group DFT (natural order in, bit-reversed out; one thread per butterfly, one scalar
// multiplication by the twiddle each, complete additions -- Curve::add handles P + P, P - P and O), the scaling pass in front of it,
// the column sums K_v over a column-major copy of C (coefficients 1 and -1 add / subtract, others multiply), and the per-proof
// elementwise pass that forms p_j and the degree check's dot product.
#pragma once
#include "bn254.hpp"
#include "common.hpp"
#include "ntt.hpp"

namespace zk {

// k * P, k a Montgomery Fr element: left-to-right double and add (once per key: no tables, no recoding)
template <class C>
static ZK_D typename C::XYZZ hl_smul(const typename C::XYZZ &P, const fe &k_mont) {
    const fe k = Fr::from_mont(k_mont);
    typename C::XYZZ acc = C::infinity();
    if (C::is_inf(P)) return acc;
    int top = 253;
    while (top >= 0 && !((k.l[top >> 5] >> (top & 31)) & 1u)) top--;
    for (int b = top; b >= 0; b--) {
        acc = C::dbl(acc);
        if ((k.l[b >> 5] >> (b & 31)) & 1u) acc = C::add(acc, P);
    }
    return acc;
}

// out[i] = scale[i] * in[i] for i < n_in, the point at infinity for n_in <= i < m
__global__ void __launch_bounds__(64)
k_gdft_scale(const G1::Affine *__restrict__ in, uint32_t n_in, const fe *__restrict__ scale, G1::XYZZ *__restrict__ out, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    out[i] = i < n_in ? hl_smul<G1>(G1::from_affine(in[i]), scale[i]) : G1::infinity();
}

// stage s (0-based) of the decimation-in-frequency transform, in place: pairs (u, u + half), half = m >> (s + 1):
//   a[u] <- a[u] + a[u + half],   a[u + half] <- tw[i << s] * (a[u] - a[u + half])      (i = u mod half; tw[k] = root^k, k < m / 2)
__global__ void __launch_bounds__(64)
k_gdft_stage(G1::XYZZ *__restrict__ a, const fe *__restrict__ tw, uint32_t logm, uint32_t s) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (1u << (logm - 1))) return;
    const uint32_t hbits = logm - 1 - s, half = 1u << hbits;
    const uint32_t i = b & (half - 1), u = ((b >> hbits) << (hbits + 1)) | i, v = u + half;
    const G1::XYZZ x = a[u], y = a[v];
    a[u] = G1::add(x, y);
    const G1::XYZZ d = G1::add(x, G1::neg(y));
    a[v] = i ? hl_smul<G1>(d, tw[(size_t)i << s]) : d;                    // w^0 = 1
}

// out[j] = affine(a[bitrev(j)]): undoes the transform's output order and normalises (canonical coordinates)
__global__ void __launch_bounds__(64)
k_gdft_finish(const G1::XYZZ *__restrict__ a, G1::Affine *__restrict__ out, uint32_t logm) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (1u << logm)) return;
    out[j] = G1::to_affine(a[bitrev32(j, logm)]);
}

// d_out[0 .. m) <- 1 / (m Z(g)) sum_{i < n_in} r^(-i) w^(-ij) d_in[i]   with r = g (coset != 0) or 1; d_work: m XYZZ points of scratch
static inline int gdft_run(const NttTables &tab, const G1::Affine *d_in, uint32_t n_in, bool coset, G1::XYZZ *d_work, G1::Affine *d_out, hipStream_t st) {
    const uint32_t logm = tab.logm, m = 1u << logm;
    if (n_in > m) return fail_msg(ZK_ERR_ARG, "group DFT: more points than the domain holds");
    ZK_LAUNCH(k_gdft_scale, zk_div_up(m, 64), 64, st, d_in, n_in, (const fe *)(coset ? tab.icoset_zinv : tab.inv_m_zinv), d_work, m);
    for (uint32_t s = 0; s < logm; s++)
        ZK_LAUNCH(k_gdft_stage, zk_div_up(m / 2, 64), 64, st, d_work, (const fe *)tab.tw_inv, logm, s);
    ZK_LAUNCH(k_gdft_finish, zk_div_up(m, 64), 64, st, (const G1::XYZZ *)d_work, d_out, logm);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// ---- K_v = sum_j C[j][v] Lambda_j over a column-major copy of C.  Columns are cut into chunks of HL_COL_CHUNK entries (the constant
// ONE and a circuit's accumulator variables stand in very many rows): one thread per chunk, then one thread per column.
constexpr uint32_t HL_COL_CHUNK = 128;
static ZK_HD bool fr_is_minus_one(const fe &a) {
    uint32_t t = 0;
    const fe mo = Fr::neg(Fr::one());
#pragma unroll
    for (int i = 0; i < 8; i++) t |= a.l[i] ^ mo.l[i];
    return t == 0;
}
__global__ void __launch_bounds__(64)
k_hl_col_chunks(const uint32_t *__restrict__ chunk_begin, const uint32_t *__restrict__ chunk_end, uint32_t n_chunks,
                const uint32_t *__restrict__ row, const fe *__restrict__ coeff, const G1::Affine *__restrict__ lambda, G1::XYZZ *__restrict__ partial) {
    const uint32_t ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_chunks) return;
    G1::XYZZ acc = G1::infinity();
    for (uint32_t k = chunk_begin[ch]; k < chunk_end[ch]; k++) {
        const G1::Affine p = lambda[row[k]];
        const fe cf = coeff[k];
        if (fr_is_one(cf)) acc = G1::madd(acc, p);                         // the add-only paths: most coefficients of a circuit are 1 or -1
        else if (fr_is_minus_one(cf)) acc = G1::madd(acc, G1::neg(p));
        else acc = G1::add(acc, hl_smul<G1>(G1::from_affine(p), cf));
    }
    partial[ch] = acc;
}
// out[v] = affine(L_v - K_v) for v < n_cols; L_v = l_bases[v - l_first] for v >= l_first, the point at infinity below
__global__ void __launch_bounds__(64)
k_hl_col_finish(const uint32_t *__restrict__ col_first_chunk, const G1::XYZZ *__restrict__ partial, const G1::Affine *__restrict__ l_bases,
                uint32_t l_first, uint32_t n_cols, G1::Affine *__restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_cols) return;
    G1::XYZZ acc = G1::infinity();
    for (uint32_t k = col_first_chunk[v]; k < col_first_chunk[v + 1]; k++) acc = G1::add(acc, partial[k]);
    acc = G1::neg(acc);
    if (v >= l_first) acc = G1::madd(acc, l_bases[v - l_first]);
    out[v] = G1::to_affine(acc);
}

// ---- per proof: the H scalars and the degree check.
// a, b: A and B on the coset, b scaled by 1 / R (its inverse transform's post-scale carries the factor), so that the Montgomery product
// a[j] b[j] IS the canonical value p_j the bucket sort wants (no conversion in the sort's two passes); c: the C row evaluations.
// h[m-1] = 1 / (m Z(g)) (g^(-(m-1)) sum_j w^j p_j - sum_j w^j c_j): every workgroup leaves its share of the two sums in part[2 (proof * grid + block) ..].
constexpr uint32_t HL_PROD_THREADS = 256;
constexpr uint32_t HL_PROD_PER = 8;             // elements per thread (strided by the workgroup): one LDS tree and one pair of partial sums per 2048 elements
__global__ void __launch_bounds__(HL_PROD_THREADS)
k_hl_product(const fe *__restrict__ a, const fe *__restrict__ b, const fe *__restrict__ c, const fe *__restrict__ tw,
             fe *__restrict__ p_out, fe *__restrict__ part, uint32_t m, uint32_t stride) {
    __shared__ uint32_t sh[2][8][HL_PROD_THREADS];
    const size_t at = (size_t)blockIdx.y * stride;
    const uint32_t half = m >> 1;
    fe sp = Fr::zero(), sc = Fr::zero();
    for (uint32_t e = 0; e < HL_PROD_PER; e++) {
        const uint32_t j = (blockIdx.x * HL_PROD_PER + e) * HL_PROD_THREADS + threadIdx.x;
        if (j >= m) break;
        const fe p = Fr::mul(a[at + j], b[at + j]);
        p_out[at + j] = p;
        fe tp = p, tc = c[at + j];
        if (half) {
            const fe w = tw[j & (half - 1)];                                // w^(j + m/2) = -w^j
            tp = Fr::mul(tp, w); tc = Fr::mul(tc, w);
            if (j >= half) { tp = Fr::neg(tp); tc = Fr::neg(tc); }
        }
        sp = Fr::add(sp, tp); sc = Fr::add(sc, tc);
    }
#pragma unroll
    for (int l = 0; l < 8; l++) { sh[0][l][threadIdx.x] = sp.l[l]; sh[1][l][threadIdx.x] = sc.l[l]; }
    __syncthreads();
    for (uint32_t s = HL_PROD_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            fe o0, o1;
#pragma unroll
            for (int l = 0; l < 8; l++) { o0.l[l] = sh[0][l][threadIdx.x + s]; o1.l[l] = sh[1][l][threadIdx.x + s]; }
            sp = Fr::add(sp, o0); sc = Fr::add(sc, o1);
#pragma unroll
            for (int l = 0; l < 8; l++) { sh[0][l][threadIdx.x] = sp.l[l]; sh[1][l][threadIdx.x] = sc.l[l]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        fe *o = part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = sp; o[1] = sc;
    }
}
// h given by its coefficients (the two-step submit, whose h comes out of the six-transform chains): q = Z(g) h + C, coefficient by
// coefficient; its coset transform gives the p_j.  h has n_h = m - 1 coefficients.
__global__ void k_hl_q_from_h(const fe *__restrict__ h, uint32_t n_h, const fe *__restrict__ c_coef, fe zg, fe *__restrict__ out, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    out[i] = i < n_h ? Fr::add(Fr::mul(h[i], zg), c_coef[i]) : c_coef[i];
}
// one workgroup per proof: tail[proof] = kp * sum(part p) - kc * sum(part c)   (kp, kc: the constants of the formula above, kp with the
// factor R^2 that takes the canonical sum to Montgomery form)
__global__ void __launch_bounds__(HL_PROD_THREADS)
k_hl_tail(const fe *__restrict__ part, uint32_t n_part, fe kp, fe kc, fe *__restrict__ tail) {
    __shared__ uint32_t sh[2][8][HL_PROD_THREADS];
    const fe *in = part + 2 * (size_t)blockIdx.x * n_part;
    fe sp = Fr::zero(), sc = Fr::zero();
    for (uint32_t k = threadIdx.x; k < n_part; k += blockDim.x) { sp = Fr::add(sp, in[2 * k]); sc = Fr::add(sc, in[2 * k + 1]); }
#pragma unroll
    for (int l = 0; l < 8; l++) { sh[0][l][threadIdx.x] = sp.l[l]; sh[1][l][threadIdx.x] = sc.l[l]; }
    __syncthreads();
    for (uint32_t s = HL_PROD_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            fe o0, o1;
#pragma unroll
            for (int l = 0; l < 8; l++) { o0.l[l] = sh[0][l][threadIdx.x + s]; o1.l[l] = sh[1][l][threadIdx.x + s]; }
            sp = Fr::add(sp, o0); sc = Fr::add(sc, o1);
#pragma unroll
            for (int l = 0; l < 8; l++) { sh[0][l][threadIdx.x] = sp.l[l]; sh[1][l][threadIdx.x] = sc.l[l]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) tail[blockIdx.x] = Fr::sub(Fr::mul(sp, kp), Fr::mul(sc, kc));
}

}  // namespace zk
