// eddsa_sign.hpp -- the device EdDSA signer (jubjub.cpp, zk_eddsa_sign_batch / zk_eddsa_sign_probe of include/zkhip.h): the native side of
// _SignatureScheme.sign of ethsnarks/eddsa.py for its three schemes.  Included from jubjub.cpp behind jubjub.hpp, whose curve arithmetic, MiMC
// cipher, Pedersen step and bit-stream reader it uses unchanged.  DESIGN 5l.
//
//   M       the message as hash_public takes it, and its bytes as to_bytes gives them: the msg_len field elements as 32 little-endian bytes each
//           (mimc), the msg_len message bytes (pure), the point pedersen_hash_bytes("EdDSA_Verify.M", msg) as x then y, 32 bytes each (hash)
//   r     = int_le(SHA-512(k as 32 little-endian bytes || bytes of M)) mod L
//   R, A  = r B, k B
//   t     = H(R, A, M) of the scheme, as k_eddsa_verify computes it
//   S     = (r + k t) mod E,  E = 8 L
//
// NOT CONSTANT TIME: the table rows read and the reductions' final subtractions depend on the secret digits.
//
// WHERE THE SECRETS LIVE.  The key stays in the device buffer the host uploaded it to and the nonce goes to a buffer beside it the moment it is
// reduced; the host zeroes both before the call returns.  The kernel holds neither in a private array (a digit taken with a runtime index would
// put the whole scalar into the lane's scratch memory, which nobody clears) and keeps neither in registers across a call (a value that is live
// across a call sits in a callee-saved register, which the callee may save to scratch): every digit is a fresh word load from the two
// buffers (secret_digit), and r and k are loaded whole only for the closing r + k t, after the last call.  What a call can still carry into
// scratch is the table address of one digit.
//
// SHA-512 streams over 128-byte blocks; the message schedule is a rolling window of 16 words whose indices are compile-time constants after
// unrolling (a W[80] indexed by the round counter would live in scratch memory); state and schedule are dead before the curve part starts.
//
// The two wide reductions are ONE Barrett reduction (HAC 14.42) in base b = 2^32 with k = 8: for x < b^16 and b^7 <= m < b^8,
// q3 = floor(floor(x / b^7) mu / b^9) with mu = floor(b^16 / m) is the quotient or up to 2 below it, so x - q3 m, computed modulo b^9, is below
// 3 m and two conditional subtractions finish.  L (251 bits) and E (254 bits) both have a non-zero top limb.  About 81 + 72 word products: less
// than two field products.
//
// R = r B and A = k B share one loop over the 64 four-bit windows, least significant first, with two accumulators and NO doublings: the handle's
// fixed-base table holds m 16^j B for m = 0 .. 15, j = 0 .. 63 as (x, y, d x y) -- entry (j 16 + m), 96 bytes each, 98 304 bytes in all; m = 0 is
// the identity, so a zero digit takes the same mixed addition as any other and the loop is uniform across the wave.  Both accumulators read row
// j in the same iteration.  One inversion of Z_R Z_A makes both points affine.
//
// Kernels (one lane per item, workgroups of 64):
//   k_eddsa_sign        n signatures
//   k_eddsa_sign_probe  the SHA-512 and the two reductions above on their own, for the tests
#pragma once
#include "jubjub.hpp"

namespace zk {
namespace jubjub {

constexpr uint32_t SIGN_TABLE_ENTRIES = N_WIN * TABLE;          // 1 024 points, 3 elements each
enum { SIGN_PROBE_SHA512 = 0, SIGN_PROBE_MOD_L = 1, SIGN_PROBE_MULADD_MOD_E = 2 };

struct wide { uint32_t l[16]; };                                // a 512-bit integer, least significant limb first

struct ModL {                                                   // the order of the prime subgroup
    ZK_HD static uint32_t m(int i) {
        constexpr uint32_t v[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
        return v[i];
    }
    ZK_HD static uint32_t mu(int i) {                           // floor(2^512 / L)
        constexpr uint32_t v[9] = {0x2ce10002u, 0xb90b6ff4u, 0xca2fbea9u, 0x1ce06fefu, 0x03980a0du, 0x83a52c34u, 0x1d0253d5u, 0x523a3131u, 0x0000002au};
        return v[i];
    }
};
struct ModE {                                                   // the order of the curve, 8 L
    ZK_HD static uint32_t m(int i) {
        constexpr uint32_t v[8] = {0xc9093788u, 0x3b94bee1u, 0xc9077053u, 0x59f76dc1u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
        return v[i];
    }
    ZK_HD static uint32_t mu(int i) {                           // floor(2^512 / E)
        constexpr uint32_t v[9] = {0x859c2000u, 0x37216dfeu, 0xf945f7d5u, 0xa39c0dfdu, 0x80730141u, 0xb074a586u, 0x23a04a7au, 0x4a474626u, 0x00000005u};
        return v[i];
    }
};

// x mod m, x any 512-bit integer.  Every loop has constant bounds and is unrolled: the limb arrays stay in registers
template <class M>
ZK_HD fe reduce_wide(const wide &x) {
    // q3 = limbs 9 .. 17 of (x >> 224) mu: a 9 x 9 limb product by columns, the columns below 9 kept only for their carries
    uint32_t q3[9];
    uint64_t lo = 0, hi = 0;                                    // the running column sum, hi counting the 2^64 overflows
#pragma unroll
    for (int col = 0; col < 18; col++) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const int j = col - i;
            if (j < 0 || j > 8) continue;
            const uint64_t p = (uint64_t)x.l[7 + i] * M::mu(j);
            lo += p;
            hi += lo < p;
        }
        if (col >= 9) q3[col - 9] = (uint32_t)lo;
        lo = (lo >> 32) | (hi << 32);
        hi = 0;
    }
    // r = (x - q3 m) mod b^9
    uint32_t r[9];
    lo = 0; hi = 0;
    uint64_t borrow = 0;
#pragma unroll
    for (int col = 0; col < 9; col++) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const int j = col - i;
            if (j < 0 || j > 7) continue;
            const uint64_t p = (uint64_t)q3[i] * M::m(j);
            lo += p;
            hi += lo < p;
        }
        const uint64_t d = (uint64_t)x.l[col] - (uint32_t)lo - borrow;
        r[col] = (uint32_t)d;
        borrow = (d >> 32) & 1;
        lo = (lo >> 32) | (hi << 32);
        hi = 0;
    }
    // at most two subtractions of m
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        uint32_t s[9];
        uint64_t b = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const uint64_t d = (uint64_t)r[i] - (i < 8 ? M::m(i) : 0u) - b;
            s[i] = (uint32_t)d;
            b = (d >> 32) & 1;
        }
        if (!b) {
#pragma unroll
            for (int i = 0; i < 9; i++) r[i] = s[i];
        }
    }
    fe o;
#pragma unroll
    for (int i = 0; i < 8; i++) o.l[i] = r[i];
    return o;
}

// a + b c as a 512-bit integer (a, b, c any 256-bit integers: the sum is below 2^512)
ZK_HD wide muladd_wide(const fe &a, const fe &b, const fe &c) {
    wide x;
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int col = 0; col < 16; col++) {
        if (col < 8) { lo += a.l[col]; hi += lo < a.l[col]; }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int j = col - i;
            if (j < 0 || j > 7) continue;
            const uint64_t p = (uint64_t)b.l[i] * c.l[j];
            lo += p;
            hi += lo < p;
        }
        x.l[col] = (uint32_t)lo;
        lo = (lo >> 32) | (hi << 32);
        hi = 0;
    }
    return x;
}

// ---- SHA-512 (FIPS 180-4) of the bytes a[0 .. alen) || b[0 .. blen); the digest as the 512-bit integer int_le(digest) -- which is also the
// digest's 64 bytes when the limbs are stored in order
ZK_HD uint64_t sha512_k(uint32_t i) {
    constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
        0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
        0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
        0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
        0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
        0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
        0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    return K[i];
}
ZK_HD uint64_t sha512_iv(int i) {
    constexpr uint64_t v[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                               0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    return v[i];
}
ZK_HD uint64_t rotr64(uint64_t x, uint32_t n) { return (x >> n) | (x << (64 - n)); }
ZK_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

ZK_HD wide sha512_le(const uint8_t *__restrict__ a, uint32_t alen, const uint8_t *__restrict__ b, uint32_t blen) {
    uint64_t H[8];
#pragma unroll
    for (int i = 0; i < 8; i++) H[i] = sha512_iv(i);
    const uint64_t total = (uint64_t)alen + blen;
    const uint64_t n_blocks = (total + 17 + 127) / 128;         // the 0x80 byte and the 16 bytes of the bit length fit in the last block
#pragma clang loop unroll(disable)
    for (uint64_t blk = 0; blk < n_blocks; blk++) {
        uint64_t W[16];
#pragma unroll
        for (int i = 0; i < 16; i++) W[i] = 0;
        // the 16 words come in through W[15] and move down one place per word: a rolled loop with eight byte loads in flight, not 128, and
        // still no runtime index into W
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < 16; i++) {
            uint64_t w = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint64_t pos = blk * 128 + 8 * i + k;
                const uint32_t byte = pos < alen ? a[pos] : pos < total ? b[pos - alen] : pos == total ? 0x80u : 0u;
                w = (w << 8) | byte;
            }
#pragma unroll
            for (int j = 0; j < 15; j++) W[j] = W[j + 1];
            W[15] = w;
        }
        if (blk == n_blocks - 1) W[15] |= total * 8;            // (total < 2^33: the upper length word stays 0)
        uint64_t S[8];
#pragma unroll
        for (int i = 0; i < 8; i++) S[i] = H[i];
#pragma clang loop unroll(disable)
        for (uint32_t r = 0; r < 80; r += 16) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (r) {
                    const uint64_t w1 = W[(i + 1) & 15], w14 = W[(i + 14) & 15];
                    W[i] += (rotr64(w1, 1) ^ rotr64(w1, 8) ^ (w1 >> 7)) + W[(i + 9) & 15] + (rotr64(w14, 19) ^ rotr64(w14, 61) ^ (w14 >> 6));
                }
                // the working variables a .. h are S[(0 - i) & 7] .. S[(7 - i) & 7]: a round renames instead of moving
                uint64_t &va = S[(0 - i) & 7], &vb = S[(1 - i) & 7], &vc = S[(2 - i) & 7], &vd = S[(3 - i) & 7];
                uint64_t &ve = S[(4 - i) & 7], &vf = S[(5 - i) & 7], &vg = S[(6 - i) & 7], &vh = S[(7 - i) & 7];
                const uint64_t t1 = vh + (rotr64(ve, 14) ^ rotr64(ve, 18) ^ rotr64(ve, 41)) + ((ve & vf) ^ (~ve & vg)) + sha512_k(r + i) + W[i];
                const uint64_t t2 = (rotr64(va, 28) ^ rotr64(va, 34) ^ rotr64(va, 39)) + ((va & vb) ^ (va & vc) ^ (vb & vc));
                vd += t1;
                vh = t1 + t2;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) H[i] += S[i];
    }
    wide o;
#pragma unroll
    for (int i = 0; i < 8; i++) { o.l[2 * i] = bswap32((uint32_t)(H[i] >> 32)); o.l[2 * i + 1] = bswap32((uint32_t)H[i]); }
    return o;
}

// digit j of a secret scalar, read from its (wiped) device buffer at every use: volatile, so that the load is neither hoisted nor shared
ZK_HD uint32_t secret_digit(const fe *x, uint32_t j) { return (((const volatile uint32_t *)x->l)[j >> 3] >> ((j & 7) * WIN)) & (TABLE - 1); }
ZK_HD fe secret_load(const fe *x) {
    fe o;
#pragma unroll
    for (int i = 0; i < 8; i++) o.l[i] = ((const volatile uint32_t *)x->l)[i];
    return o;
}

// A[g], R[g], s[g] = the signature of msgs[g] under keys[g]; canonical integers.  ftab: the SIGN_TABLE_ENTRIES x (x, y, d x y) of m 16^j B.
// The host has checked 0 < key < L and every MiMC message element < r.  nonces: n elements, r of each item, zeroed by the host with the keys.
// mpt (ZK_EDDSA_HASH only): n x 2 elements, M of each item
__global__ void __launch_bounds__(BLOCK)
k_eddsa_sign(EddsaView v, const fe *__restrict__ ftab, const fe *keys, fe *nonces, const void *__restrict__ msgs, uint32_t n, fe *A, fe *R, fe *__restrict__ s, fe *mpt) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;

    // ---- M and its bytes
    const uint8_t *mb;
    uint32_t mlen;
    if (v.scheme == SCHEME_MIMC) {
        mb = (const uint8_t *)((const fe *)msgs + (size_t)g * v.msg_len); mlen = 32 * v.msg_len;   // (canonical limbs in memory ARE the 32 little-endian bytes)
    } else if (v.scheme == SCHEME_PURE) {
        mb = (const uint8_t *)msgs + (size_t)g * v.msg_len; mlen = v.msg_len;
    } else {
        const uint8_t *__restrict__ m = (const uint8_t *)msgs + (size_t)g * v.msg_len;
        jpoint acc;
        set_identity(acc);
#pragma clang loop unroll(disable)
        for (uint32_t j = 0; j < v.m_windows; j++) {
            uint32_t w = 0;
            for (uint32_t b = 0; b < 3; b++) { const uint32_t i = 3 * j + b; if (i < 8 * v.msg_len) w |= ((m[i >> 3] >> (7 - (i & 7))) & 1u) << b; }
            pedersen_step(acc, v.m_tab, j, w);
        }
        fe mx, my;
        to_affine_int(acc, mx, my);
        mpt[2 * (size_t)g] = mx; mpt[2 * (size_t)g + 1] = my;
        mb = (const uint8_t *)(mpt + 2 * (size_t)g); mlen = 64;
    }

    // ---- the nonce: straight from the reduction to its buffer (no call between the first key byte read and this store)
    {
        const fe r = reduce_wide<ModL>(sha512_le((const uint8_t *)(keys + g), 32, mb, mlen));
#pragma unroll
        for (int i = 0; i < 8; i++) ((volatile uint32_t *)nonces[g].l)[i] = r.l[i];
    }

    // ---- R = r B, A = k B
    jpoint pr, pa;
    set_identity(pr);
    set_identity(pa);
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < N_WIN; j++) {
        const fe *__restrict__ row = ftab + (size_t)j * TABLE * 3;
        jj_add(pr, row + 3 * secret_digit(nonces + g, j), true);
        jj_add(pa, row + 3 * secret_digit(keys + g, j), true);
    }
    fe rx, ry, ax, ay;                                          // Montgomery
    {
        const fe zi = jj_inv(jj_mul(pr.c[3], pa.c[3]));
        const fe zr = jj_mul(zi, pa.c[3]), za = jj_mul(zi, pr.c[3]);
        rx = jj_mul(pr.c[0], zr); ry = jj_mul(pr.c[1], zr);
        ax = jj_mul(pa.c[0], za); ay = jj_mul(pa.c[1], za);
    }
    fe *Rg = R + 2 * (size_t)g, *Ag = A + 2 * (size_t)g;
    Rg[0] = jj_from_mont(rx); Rg[1] = jj_from_mont(ry);
    Ag[0] = jj_from_mont(ax); Ag[1] = jj_from_mont(ay);

    // ---- t = H(R, A, M), as k_eddsa_verify
    fe t;                                                       // the canonical integer
    if (v.scheme == SCHEME_MIMC) {
        const fe *__restrict__ m = (const fe *)msgs + (size_t)g * v.msg_len;
        fe key = Fr::zero();
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < 4 + v.msg_len; i++) {
            const fe xi = i == 0 ? rx : i == 1 ? ry : i == 2 ? ax : i == 3 ? ay : jj_to_mont(m[i - 4]);
            key = Fr::ladd(Fr::ladd(key, xi), jj_mimc_cipher(v.rc, xi, key));
        }
        t = jj_from_mont(key);
    } else {
        BitStream bs;                                           // the canonical R.x and A.x are read back from the lane's own output
        bs.rx = Rg[0].l; bs.ax = Ag[0].l; bs.mx = v.scheme == SCHEME_HASH ? mpt[2 * (size_t)g].l : nullptr;
        bs.msg = (const uint8_t *)msgs + (size_t)g * v.msg_len; bs.msg_bits = 8 * v.msg_len;
        jpoint acc;
        set_identity(acc);
#pragma clang loop unroll(disable)
        for (uint32_t j = 0; j < v.ram_windows; j++) pedersen_step(acc, v.ram_tab, j, bs.window(j));
        fe ty;
        to_affine_int(acc, t, ty);
    }

    // ---- S = (r + k t) mod E: r and k come into registers here, behind the last call of the kernel
    s[g] = reduce_wide<ModE>(muladd_wide(secret_load(nonces + g), secret_load(keys + g), t));
}

// the device functions of the signer on their own: op 0: out[g] = SHA-512 of the len bytes at a + g len (16 words); op 1: out[g] = the
// 512-bit integer a[g] mod L (8 words); op 2: out[g] = (a[g] + b[g] c[g]) mod E (8 words)
__global__ void __launch_bounds__(BLOCK)
k_eddsa_sign_probe(int op, const void *__restrict__ a, const fe *__restrict__ b, const fe *__restrict__ c, uint32_t n, uint32_t len, uint32_t *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    if (op == SIGN_PROBE_SHA512) {
        const wide d = sha512_le(nullptr, 0, (const uint8_t *)a + (size_t)g * len, len);
        for (int i = 0; i < 16; i++) out[16 * (size_t)g + i] = d.l[i];
    } else if (op == SIGN_PROBE_MOD_L) {
        const fe o = reduce_wide<ModL>(((const wide *)a)[g]);
        for (int i = 0; i < 8; i++) out[8 * (size_t)g + i] = o.l[i];
    } else {
        const fe o = reduce_wide<ModE>(muladd_wide(((const fe *)a)[g], b[g], c[g]));
        for (int i = 0; i < 8; i++) out[8 * (size_t)g + i] = o.l[i];
    }
}

}  // namespace jubjub
}  // namespace zk
