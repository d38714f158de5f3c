// jubjub.hpp -- Baby JubJub on the device: curve arithmetic, the windowed Pedersen hash and batch EdDSA verification (jubjub.cpp, zk_jj_*,
// zk_pedersen_*, zk_eddsa_* of include/zkhip.h).  The native side of ethsnarks/jubjub.py, pedersen.py and eddsa.py, and the witness of the
// MiMC-EdDSA circuit whose gadgets are ethsnarks_amd/jubjub_gadgets.py.
//
// The curve is the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr with a = 168700 (a square) and d = 168696 (a non-square), so the
// unified addition below is COMPLETE: no input pair on the curve makes a denominator vanish, Z stays non-zero, and the identity, P = Q, P = -Q and
// the eight low-order points all go through the same instructions.  Points are extended (X : Y : T : Z), x = X/Z, y = Y/Z, T = XY/Z, in the loose
// Montgomery domain of bn254.hpp.
//
//   addition (EtecPoint.add, HWCD 2008 section 3.1):  A = X1 X2, B = Y1 Y2, C = (d T1) T2, D = Z1 Z2, E = (X1 + Y1)(X2 + Y2) - A - B, F = D - C,
//                                                     G = D + C, H = B - a A;  X3 = E F, Y3 = G H, T3 = E H, Z3 = F G
//   doubling (EtecPoint.double, dbl-2008-hwcd):       A = X^2, B = Y^2, C = 2 Z^2, D = a A, E = (X + Y)^2 - A - B, G = D + B, F = G - C, H = D - B;
//                                                     the same four products
// The second operand of an addition is always a TABLE point, kept in "addend form" (X, Y, d T, Z): the product by d is paid once per table entry
// instead of once per addition (10 products).  A table point with Z = 1 -- every point of the Pedersen and fixed-base tables -- is three elements
// (x, y, d x y) and skips D = Z1 (9 products: the mixed addition).  A doubling is 9 products, 8 when the T it would produce is not read (the next
// step is another doubling).  The products by a and d go through Fr::lmul with a Montgomery constant: see DESIGN 5h.
//
// Code size.  jj_add and jj_dbl are real functions, one body each; inside, the four coordinate products and the four output products are ROLLED
// loops over small arrays, so a body holds four copies of the field product, not ten.  Every product off the hot path (conversions, the curve
// equation, the inversion, table set-up) goes through the one body of jj_mul.
//
// Kernels (one lane per item, workgroups of 64):
//   k_jj_scalar_mul   n variable-base multiplications, 4-bit windows, a 16-entry table per lane (private memory), scalars of 256 bits
//   k_jj_point_op     n additions / doublings / negations of affine points
//   k_jj_pedersen     n windowed Pedersen hashes over a table of affine multiples in device memory, the window count per lane
//   k_eddsa_verify    n verdicts S B == R + t A, t = H(R, A, M) computed here for the three schemes of eddsa.py
//   k_eddsa_fill      n complete witness rows of the MiMC-EdDSA circuit, one field inversion per row
//   k_eddsa_fill_wide the same rows with 2 or 4 lanes per witness, one per wave of a workgroup of 2 or 4 waves: a shorter dependent chain
//   k_eddsa_fill_pure n complete witness rows of the PureEdDSA circuit (in-circuit Pedersen hash), two field inversions per row
//   k_eddsa_fill_hash n complete witness rows of the EdDSA circuit (the message hashed in the circuit first), three field inversions per row (at the end of this file)
#pragma once
#include "bn254.hpp"
#include "mimc.hpp"

namespace zk {
namespace jubjub {

constexpr uint32_t BLOCK = 64;
constexpr uint32_t WIN = 4, TABLE = 1u << WIN, N_WIN = 256 / WIN;   // scalar multiplication: 64 windows of 4 bits cover any 256-bit scalar
constexpr uint32_t SEG_WINDOWS = 62;                            // Pedersen: windows per base point (pedersen.py:35)
constexpr uint32_t FIELD_BITS = 254;                            // FQ.bits(): ceil(log2 r) bits, least significant first
enum { OP_ADD = 0, OP_DOUBLE = 1, OP_NEGATE = 2 };
enum { SCHEME_MIMC = 0, SCHEME_PURE = 1, SCHEME_HASH = 2 };

#define ZK_JFN inline ZK_HD_NOINLINE

struct jpoint { fe c[4]; };                                     // X, Y, T (or d T: addend form), Z

ZK_HD fe coef_a() {                                             // 168700 R mod r
    constexpr uint32_t v[8] = {0xfff261e0u, 0x95accf61u, 0x9df7d378u, 0x24780d65u, 0x7e906ae8u, 0xe0ac11b0u, 0x16d3def3u, 0x0f35db22u};
    fe r; for (int i = 0; i < 8; i++) r.l[i] = v[i]; return r;
}
ZK_HD fe coef_d() {                                             // 168696 R mod r
    constexpr uint32_t v[8] = {0xaff261f5u, 0x2735f484u, 0x9a2e0f63u, 0x70ba1b57u, 0x1e2caa8cu, 0xff41c9a9u, 0x8fe6025fu, 0x07704a8eu};
    fe r; for (int i = 0; i < 8; i++) r.l[i] = v[i]; return r;
}

// the one product body of everything that is not the inside of jj_add / jj_dbl / the MiMC rounds
ZK_JFN fe jj_mul(const fe &a, const fe &b) { return Fr::lmul(a, b); }
ZK_HD fe jj_to_mont(const fe &a) { fe r2; for (int i = 0; i < 8; i++) r2.l[i] = FrParams::r2(i); return jj_mul(a, r2); }
// loose Montgomery -> the canonical integer
ZK_HD fe jj_from_mont(const fe &a) { fe o = Fr::zero(); o.l[0] = 1; return Fr::canon(jj_mul(a, o)); }

ZK_HD void set_identity(jpoint &p) { p.c[0] = Fr::zero(); p.c[1] = Fr::one(); p.c[2] = Fr::zero(); p.c[3] = Fr::one(); }

// p <- p + q.  q: X, Y, d T and -- unless mixed -- Z of the addend; mixed: Z2 = 1 and q has three elements
ZK_JFN void jj_add(jpoint &p, const fe *q, bool mixed) {
    fe m[4];
    const uint32_t np = mixed ? 3 : 4;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < np; i++) m[i] = Fr::lmul(p.c[i], q[i]);   // X1 X2, Y1 Y2, d T1 T2, Z1 Z2
    if (mixed) m[3] = p.c[3];
    const fe s = Fr::lmul(Fr::ladd(p.c[0], p.c[1]), Fr::ladd(q[0], q[1]));
    const fe e = Fr::lsub(Fr::lsub(s, m[0]), m[1]);
    const fe f = Fr::lsub(m[3], m[2]), g = Fr::ladd(m[3], m[2]);
    const fe h = Fr::lsub(m[1], Fr::lmul(coef_a(), m[0]));
    fe l[4], r[4];
    l[0] = e; r[0] = f; l[1] = g; r[1] = h; l[2] = e; r[2] = h; l[3] = f; r[3] = g;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < 4; i++) p.c[i] = Fr::lmul(l[i], r[i]);
}

// p <- 2 p; need_t false: T is left as it was (stale) -- for a doubling that is followed by another doubling, which does not read it
ZK_JFN void jj_dbl(jpoint &p, bool need_t) {
    fe q[3];
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < 3; i++) { const fe &v = p.c[i == 2 ? 3 : i]; q[i] = Fr::lmul(v, v); }   // X^2, Y^2, Z^2
    const fe t = Fr::ladd(p.c[0], p.c[1]);
    const fe e = Fr::lsub(Fr::lsub(Fr::lmul(t, t), q[0]), q[1]);
    const fe d = Fr::lmul(coef_a(), q[0]);
    const fe g = Fr::ladd(d, q[1]), f = Fr::lsub(g, Fr::ldbl(q[2])), h = Fr::lsub(d, q[1]);
    fe l[4], r[4];
    l[0] = e; r[0] = f; l[1] = g; r[1] = h; l[2] = f; r[2] = g; l[3] = e; r[3] = h;     // X, Y, Z, then T
    const uint32_t np = need_t ? 4 : 3;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < np; i++) p.c[i == 2 ? 3 : i == 3 ? 2 : i] = Fr::lmul(l[i], r[i]);
}

// a^(r - 2): 253 squarings and the products of the set bits, two product bodies in a rolled loop.  0 -> 0 (never asked for: Z != 0 on the curve)
ZK_JFN fe jj_inv(const fe &a) {
    fe acc = Fr::one(), base = a;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < FIELD_BITS; i++) {
        const uint32_t w = FrParams::p(0) - 2;                  // r - 2 differs from r in its lowest limb only (no borrow)
        const uint32_t limb = i < 32 ? w : i < 64 ? FrParams::p(1) : i < 96 ? FrParams::p(2) : i < 128 ? FrParams::p(3) : i < 160 ? FrParams::p(4)
                            : i < 192 ? FrParams::p(5) : i < 224 ? FrParams::p(6) : FrParams::p(7);
        if ((limb >> (i & 31)) & 1) acc = Fr::lmul(acc, base);
        base = Fr::lmul(base, base);
    }
    return acc;
}

// affine (x, y) in Montgomery form -> extended with T = x y
ZK_HD void from_affine(jpoint &p, const fe &x, const fe &y) { p.c[0] = x; p.c[1] = y; p.c[2] = jj_mul(x, y); p.c[3] = Fr::one(); }
// the canonical integers x = X / Z, y = Y / Z: the identity comes out as (0, 1) whichever representative of zero X holds
ZK_HD void to_affine_int(const jpoint &p, fe &x, fe &y) {
    const fe zi = jj_inv(p.c[3]);
    x = jj_from_mont(jj_mul(p.c[0], zi));
    y = jj_from_mont(jj_mul(p.c[1], zi));
}
// a x^2 + y^2 == 1 + d x^2 y^2 (Montgomery in; compared canonical)
ZK_HD bool on_curve(const fe &x, const fe &y) {
    const fe x2 = jj_mul(x, x), y2 = jj_mul(y, y);
    const fe lhs = Fr::ladd(jj_mul(coef_a(), x2), y2), rhs = Fr::ladd(Fr::one(), jj_mul(coef_d(), jj_mul(x2, y2)));
    return Fr::eq(Fr::canon(lhs), Fr::canon(rhs));
}
// projective p == affine (x, y): cross-multiplied, canonical on both sides (a zero held as r compares equal to 0)
ZK_HD bool equals_affine(const jpoint &p, const fe &x, const fe &y) {
    return Fr::eq(Fr::canon(p.c[0]), Fr::canon(jj_mul(x, p.c[3]))) && Fr::eq(Fr::canon(p.c[1]), Fr::canon(jj_mul(y, p.c[3])));
}

// tab[i] = i (x, y) in addend form, i = 0 .. 15 (tab[0] = the identity: the complete addition needs no "digit is zero" branch)
ZK_HD void build_table(jpoint *tab, const fe &x, const fe &y) {
    set_identity(tab[0]);
    from_affine(tab[1], x, y);
    fe q[3];
    q[0] = x; q[1] = y; q[2] = jj_mul(coef_d(), tab[1].c[2]);
#pragma clang loop unroll(disable)
    for (uint32_t i = 2; i < TABLE; i++) { tab[i] = tab[i - 1]; jj_add(tab[i], q, true); }
#pragma clang loop unroll(disable)
    for (uint32_t i = 1; i < TABLE; i++) tab[i].c[2] = jj_mul(coef_d(), tab[i].c[2]);
}
ZK_HD uint32_t digit(const uint32_t *limbs, uint32_t j) { return (limbs[j >> 3] >> ((j & 7) * WIN)) & (TABLE - 1); }

ZK_HD void load_point(const fe *__restrict__ src, size_t g, fe &x, fe &y) { x = jj_to_mont(src[2 * g]); y = jj_to_mont(src[2 * g + 1]); }

// out[g] = k[g] (pts[g]); canonical affine in and out, k = any 256-bit integer.  A point off the curve: *bad += 1 and nothing written
__global__ void __launch_bounds__(BLOCK)
k_jj_scalar_mul(const fe *__restrict__ pts, const fe *__restrict__ k, uint32_t n, fe *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe x, y;
    load_point(pts, g, x, y);
    if (!on_curve(x, y)) { atomicAdd(bad, 1u); return; }
    jpoint tab[TABLE];
    build_table(tab, x, y);
    jpoint acc;
    set_identity(acc);
    const uint32_t *__restrict__ kw = k[g].l;
#pragma clang loop unroll(disable)
    for (int j = N_WIN - 1; j >= 0; j--) {
#pragma clang loop unroll(disable)
        for (uint32_t b = 0; b < WIN; b++) jj_dbl(acc, b == WIN - 1);
        jj_add(acc, tab[digit(kw, j)].c, false);
    }
    to_affine_int(acc, out[2 * (size_t)g], out[2 * (size_t)g + 1]);
}

// out[g] = p[g] + q[g] (the unified addition, not the doubling, whatever the operands), 2 p[g] (the doubling) or -p[g]
__global__ void __launch_bounds__(BLOCK)
k_jj_point_op(int op, const fe *__restrict__ p, const fe *__restrict__ q, uint32_t n, fe *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe x, y;
    load_point(p, g, x, y);
    bool ok = on_curve(x, y);
    jpoint a;
    from_affine(a, x, y);
    if (op == OP_ADD) {
        jpoint b;
        load_point(q, g, x, y);
        ok = ok && on_curve(x, y);
        from_affine(b, x, y);
        b.c[2] = jj_mul(coef_d(), b.c[2]);
        if (ok) jj_add(a, b.c, false);
    } else if (op == OP_DOUBLE) {
        if (ok) jj_dbl(a, true);
    } else {
        a.c[0] = Fr::lneg(a.c[0]);
    }
    if (!ok) { atomicAdd(bad, 1u); return; }
    to_affine_int(a, out[2 * (size_t)g], out[2 * (size_t)g + 1]);
}

// ---- the windowed Pedersen hash (pedersen_hash_windows).  table[(j 4 + m) 3 ..] = (x, y, d x y) of (m + 1) 16^(j % 62) B_(j / 62), Montgomery,
// canonical; window w of position j adds entry (w & 3), negated when w > 3
ZK_HD void pedersen_step(jpoint &acc, const fe *__restrict__ table, uint32_t j, uint32_t w) {
    const fe *__restrict__ e = table + ((size_t)j * 4 + (w & 3)) * 3;
    const bool neg = w > 3;
    fe q[3];
    q[0] = neg ? Fr::lneg(e[0]) : e[0];
    q[1] = e[1];
    q[2] = neg ? Fr::lneg(e[2]) : e[2];
    jj_add(acc, q, true);
}

// out[g] = the hash of the windows win[g stride .. g stride + count - 1], count = counts[g] (or stride: counts == nullptr); canonical affine.
// The host has checked every window (<= 7) and count (1 .. min(stride, capacity)); lanes of a wave may run different counts
__global__ void __launch_bounds__(BLOCK)
k_jj_pedersen(const fe *__restrict__ table, const uint8_t *__restrict__ win, const uint32_t *__restrict__ counts, uint32_t stride, uint32_t n, fe *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t cnt = counts ? counts[g] : stride;
    const uint8_t *__restrict__ w = win + (size_t)g * stride;
    jpoint acc;
    set_identity(acc);
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < cnt; j++) pedersen_step(acc, table, j, w[j]);
    to_affine_int(acc, out[2 * (size_t)g], out[2 * (size_t)g + 1]);
}

// ---- EdDSA.  The bit stream of PureEdDSA / EdDSA.hash_public: bits(R.x) || bits(A.x) || M, a field element as 254 bits least significant
// first, message bytes most significant bit first, M of the hash scheme the x of a point (254 bits); past the end: zeros (the padding of
// the last window).  rx, ax, mx: canonical integers as limbs
struct BitStream {
    const uint32_t *rx, *ax, *mx;
    const uint8_t *msg;
    uint32_t msg_bits;
    ZK_HD static uint32_t field_bit(const uint32_t *v, uint32_t i) { return (v[i >> 5] >> (i & 31)) & 1; }
    ZK_HD uint32_t bit(uint32_t i) const {
        if (i < FIELD_BITS) return field_bit(rx, i);
        i -= FIELD_BITS;
        if (i < FIELD_BITS) return field_bit(ax, i);
        i -= FIELD_BITS;
        if (mx) return i < FIELD_BITS ? field_bit(mx, i) : 0;
        return i < msg_bits ? (msg[i >> 3] >> (7 - (i & 7))) & 1 : 0;
    }
    ZK_HD uint32_t window(uint32_t j) const { return bit(3 * j) | (bit(3 * j + 1) << 1) | (bit(3 * j + 2) << 2); }
};

// what the verify kernel knows of a verifier: btab = i B, i = 0 .. 15, as (x, y, d x y) (entry 0 = the identity (0, 1, 0)); rc = the 91 MiMC
// constants of seed "EdDSA_Verify.RAM"; ram_tab / m_tab = the Pedersen tables of "EdDSA_Verify.RAM" / "EdDSA_Verify.M"
struct EddsaView {
    const fe *btab, *rc, *ram_tab, *m_tab;
    uint32_t scheme, msg_len, ram_windows, m_windows;
};

ZK_JFN fe jj_mimc_cipher(const fe *__restrict__ rc, const fe &x, const fe &k) { return merkle::mimc_cipher(rc, x, k); }

// verdicts[g] = (s[g] B == R[g] + t A[g]) with t = H(R, A, M) of the scheme; 0 when A or R is not on the curve.  Straus: the 256 doublings are
// shared, every window adds one multiple of B (the shared table, mixed addition) and one of -A (the lane's own table)
__global__ void __launch_bounds__(BLOCK)
k_eddsa_verify(EddsaView v, const fe *__restrict__ A, const fe *__restrict__ R, const fe *__restrict__ s, const void *__restrict__ msgs, uint32_t n, uint8_t *__restrict__ verdicts) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe ax, ay, rx, ry;
    load_point(A, g, ax, ay);
    load_point(R, g, rx, ry);
    if (!on_curve(ax, ay) || !on_curve(rx, ry)) { verdicts[g] = 0; return; }
    fe t;                                                       // the canonical integer
    if (v.scheme == SCHEME_MIMC) {
        const fe *__restrict__ m = (const fe *)msgs + (size_t)g * v.msg_len;
        fe k = Fr::zero();
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < 4 + v.msg_len; i++) {
            const fe xi = i == 0 ? rx : i == 1 ? ry : i == 2 ? ax : i == 3 ? ay : jj_to_mont(m[i - 4]);
            k = Fr::ladd(Fr::ladd(k, xi), jj_mimc_cipher(v.rc, xi, k));
        }
        t = jj_from_mont(k);
    } else {
        const uint8_t *__restrict__ m = (const uint8_t *)msgs + (size_t)g * v.msg_len;
        jpoint acc;
        fe mx, my;
        if (v.scheme == SCHEME_HASH) {                          // M = pedersen_hash_bytes("EdDSA_Verify.M", msg)
            set_identity(acc);
#pragma clang loop unroll(disable)
            for (uint32_t j = 0; j < v.m_windows; j++) {
                uint32_t w = 0;
                for (uint32_t b = 0; b < 3; b++) { const uint32_t i = 3 * j + b; if (i < 8 * v.msg_len) w |= ((m[i >> 3] >> (7 - (i & 7))) & 1u) << b; }
                pedersen_step(acc, v.m_tab, j, w);
            }
            to_affine_int(acc, mx, my);
        }
        BitStream bs;
        bs.rx = R[2 * (size_t)g].l; bs.ax = A[2 * (size_t)g].l; bs.mx = v.scheme == SCHEME_HASH ? mx.l : nullptr; bs.msg = m; bs.msg_bits = 8 * v.msg_len;
        set_identity(acc);
#pragma clang loop unroll(disable)
        for (uint32_t j = 0; j < v.ram_windows; j++) pedersen_step(acc, v.ram_tab, j, bs.window(j));
        to_affine_int(acc, t, my);
    }
    jpoint tab[TABLE];
    build_table(tab, Fr::lneg(ax), ay);                        // multiples of -A
    jpoint acc;
    set_identity(acc);
    const uint32_t *__restrict__ sw = s[g].l;
#pragma clang loop unroll(disable)
    for (int j = N_WIN - 1; j >= 0; j--) {
#pragma clang loop unroll(disable)
        for (uint32_t b = 0; b < WIN; b++) jj_dbl(acc, b == WIN - 1);
        jj_add(acc, v.btab + 3 * (size_t)digit(sw, j), true);
        jj_add(acc, tab[digit(t.l, j)].c, false);
    }
    verdicts[g] = equals_affine(acc, rx, ry) ? 1 : 0;
}

// ---- the complete witness of the MiMC-EdDSA circuit (ethsnarks_amd/jubjub_gadgets.py, eddsa_mimc_circuit): one lane per signature writes its
// row of the device witness buffer.  FillLayout is zk_eddsa_layout of zkhip.h: the front end defines the row, the kernel takes every offset from
// it.  The host has checked that the segments lie inside the row and do not overlap.
//
// ONE inversion per witness.  The circuit's point gadgets (PointDoubler, PointAdder) name the AFFINE result of every step of three chains: the
// 253 doublings of A, the 253 additions of the variable-base multiplication, the 126 additions of the fixed-base one -- plus the three
// doublings of the validator and the closing R + t A.  The lane walks every chain in extended coordinates (jj_dbl / jj_add: complete, so no
// step has a special case) and parks (X, Y) of each step in the step's own x3, y3 slots, Z in its first slot and the running product of all
// Z so far in its second.  After one jj_inv of the final product the steps are visited backwards (Montgomery's trick: 1 / Z_i = inverse *
// prefix_i, inverse *= Z_i) and x3, y3 become affine; a last forward pass fills each gadget's products of affine inputs (alpha .. delta,
// beta .. tau) and the conditional points.  The 1 / x of NotLowOrder's IsNonZero joins the same product (its Y and M slots hold the prefix and
// the value).  Per witness, msg_len = 1: 14 816 field products, of which 381 are the inversion.
struct FillLayout {
    uint32_t msg_len, n_vars, ax_var, msg_var0, rx_var, s_bit0, iv_var, validator_var0, window_var0, fixed_adder_var0, mimc_var0, t_bit0,
             t_range_var0, cond0_var, doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0;
};
constexpr uint32_t FB_WINDOWS = FIELD_BITS / 2, N_STEPS = FIELD_BITS - 1;   // 127 two-bit windows of s; 253 doubler / conditional / adder steps
constexpr uint32_t DBL_VARS = 6, ADD_VARS = 7, VALIDATOR_VARS = 3 * DBL_VARS + 4, T_BITS_VARS = 3 * FIELD_BITS - 1, T_RANGE_VARS = 99;
constexpr uint32_t MIMC_ROUND_VARS = 4 * merkle::MIMC_ROUNDS;

ZK_HD uint32_t int_bit(const uint32_t *v, uint32_t i) { return (v[i >> 5] >> (i & 31)) & 1; }
// bit i of r - 1 (r is odd: only the lowest limb differs from r's)
ZK_HD uint32_t modulus_m1_bit(uint32_t i) {
    const uint32_t limb = i < 32 ? FrParams::p(0) - 1 : i < 64 ? FrParams::p(1) : i < 96 ? FrParams::p(2) : i < 128 ? FrParams::p(3) : i < 160 ? FrParams::p(4)
                        : i < 192 ? FrParams::p(5) : i < 224 ? FrParams::p(6) : FrParams::p(7);
    return (limb >> (i & 31)) & 1;
}
ZK_HD fe bit_fe(uint32_t b) { return b ? Fr::one() : Fr::zero(); }
ZK_HD fe neg_if(const fe &a, bool neg) { return neg ? Fr::lneg(a) : a; }

// one step of a chain: park the projective point in the gadget's block of nv variables and take its Z into the running product
ZK_JFN void park_point(fe *blk, uint32_t nv, const jpoint &p, fe &run) {
    blk[nv - 2] = p.c[0]; blk[nv - 1] = p.c[1]; blk[0] = p.c[3]; blk[1] = run;
    run = Fr::lmul(run, p.c[3]);
}
// the way back: inv = 1 / (the product up to and including this step) on entry, 1 / (the product before it) on return
ZK_JFN void unpark_point(fe *blk, uint32_t nv, fe &inv) {
    const fe zi = Fr::lmul(inv, blk[1]);
    inv = Fr::lmul(inv, blk[0]);
    blk[nv - 2] = Fr::canon(Fr::lmul(blk[nv - 2], zi));
    blk[nv - 1] = Fr::canon(Fr::lmul(blk[nv - 1], zi));
}
// PointDoubler's alpha = x x, beta = y y, gamma = d alpha beta, delta = 2 x y
ZK_JFN void fill_doubler(fe *blk, const fe &x, const fe &y) {
    const fe al = Fr::lmul(x, x), be = Fr::lmul(y, y), xy = Fr::lmul(x, y);
    blk[0] = Fr::canon(al); blk[1] = Fr::canon(be);
    blk[2] = Fr::canon(Fr::lmul(Fr::lmul(coef_d(), al), be));
    blk[3] = Fr::canon(Fr::ldbl(xy));
}
// PointAdder's beta = x1 y2, gamma = y1 x2, delta = y1 y2, epsilon = x1 x2, tau = delta epsilon
ZK_JFN void fill_adder(fe *blk, const fe &x1, const fe &y1, const fe &x2, const fe &y2) {
    const fe de = Fr::lmul(y1, y2), ep = Fr::lmul(x1, x2);
    blk[0] = Fr::canon(Fr::lmul(x1, y2)); blk[1] = Fr::canon(Fr::lmul(y1, x2));
    blk[2] = Fr::canon(de); blk[3] = Fr::canon(ep);
    blk[4] = Fr::canon(Fr::lmul(de, ep));
}
// one element through the cipher with its 91 x (a, b, c, d) stored (MiMCe7_round: a = t^2, b = a^2, c = a b, d = c t, the last d + k); E_k(x) + k
ZK_JFN fe mimc_cipher_rounds(const fe *__restrict__ rc, const fe &x0, const fe &k, fe *rounds) {
    fe x = x0;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < merkle::MIMC_ROUNDS; i++) {
        const fe t = Fr::ladd(Fr::ladd(x, k), rc[i]);
        const fe a = Fr::lmul(t, t), b = Fr::lmul(a, a), c = Fr::lmul(a, b);
        x = Fr::lmul(c, t);
        if (i == merkle::MIMC_ROUNDS - 1) x = Fr::ladd(x, k);
        fe *o = rounds + 4 * i;
        o[0] = Fr::canon(a); o[1] = Fr::canon(b); o[2] = Fr::canon(c); o[3] = Fr::canon(x);
    }
    return x;
}
// field2bits_strict and BitsNotAbove(bits, r - 1) of the canonical integer t: 254 bits, 253 results, 254 comparisons at tb; 99 products at range
ZK_JFN void fill_strict_bits(fe *tb, fe *range, const uint32_t *t) {
    fe *res = tb + FIELD_BITS, *cmp = res + (FIELD_BITS - 1);
    uint32_t run = 1, eq = int_bit(t, FIELD_BITS - 1), slot = 0;
#pragma clang loop unroll(disable)
    for (int i = FIELD_BITS - 1; i >= 0; i--) {                 // from the top bit down
        const uint32_t b = int_bit(t, i), c = modulus_m1_bit(i) ? 1u : b;
        tb[i] = bit_fe(b); cmp[i] = bit_fe(c);
        run &= c;
        if (i < (int)FIELD_BITS - 1) res[i] = bit_fe(run);      // results[i] = comparisons[i] * results[i + 1] (results[253] = comparisons[253])
        if (i < (int)FIELD_BITS - 1 && i > 0 && modulus_m1_bit(i)) { eq &= b; range[slot++] = bit_fe(eq); }
    }
}

// ---- what the rows of the three circuits (FillLayout, PureLayout, HashLayout) have in common, written once: the inputs, the validator with
// NotLowOrder, the fixed-base chain, the variable-base chains with the closing R + t A, their ways back and their gadgets' products.  Every
// piece takes the row and a ChainLayout, the twelve offsets that all three layouts hold; the four fill kernels are their own hash, the order
// of their inversions, and calls of these
struct ChainLayout {
    uint32_t ax_var, rx_var, s_bit0, validator_var0, window_var0, fixed_adder_var0, cond0_var, doubler_var0, cond_var0, adder_var0, step_stride,
             last_adder_var0;
};
template <class Layout> ZK_HD ChainLayout chain_layout(const Layout &L) {
    return {L.ax_var, L.rx_var, L.s_bit0, L.validator_var0, L.window_var0, L.fixed_adder_var0, L.cond0_var, L.doubler_var0, L.cond_var0, L.adder_var0,
            L.step_stride, L.last_adder_var0};
}

// item g: A and R in canonical Montgomery form; false when A or R is off the curve or s >= 2^254 (verdict 0, the row is not touched)
ZK_HD bool fill_load_item(const fe *__restrict__ A, const fe *__restrict__ R, const fe *__restrict__ s, size_t g, fe &ax, fe &ay, fe &rx, fe &ry) {
    load_point(A, g, ax, ay);
    load_point(R, g, rx, ry);
    const bool live = on_curve(ax, ay) && on_curve(rx, ry) && !(s[g].l[7] >> 30);
    ax = Fr::canon(ax); ay = Fr::canon(ay); rx = Fr::canon(rx); ry = Fr::canon(ry);
    return live;
}
// ONE, A, R and the 254 bits of s
ZK_HD void fill_inputs(fe *row, const ChainLayout &C, const fe &ax, const fe &ay, const fe &rx, const fe &ry, const uint32_t *__restrict__ sw) {
    row[0] = Fr::one();
    row[C.ax_var] = ax; row[C.ax_var + 1] = ay; row[C.rx_var] = rx; row[C.rx_var + 1] = ry;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < FIELD_BITS; i++) row[C.s_bit0 + i] = bit_fe(int_bit(sw, i));
}

// the fixed segment, projective: the validator's three doublings of R, the x of 8 R, and the 126 additions of s B parked behind them on `run`.
// fbtab: FB_WINDOWS x 4 entries (x, y, d x y) of m 4^i B, m = 0 .. 3 (m = 0: the identity), canonical Montgomery
ZK_HD void fixed_forward(fe *row, const ChainLayout &C, const fe *__restrict__ fbtab, const fe &rx, const fe &ry, const uint32_t *__restrict__ sw, fe &run) {
    fe *val = row + C.validator_var0;
    jpoint p;
    from_affine(p, rx, ry);
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < 3; j++) { jj_dbl(p, false); park_point(val + DBL_VARS * j, DBL_VARS, p, run); }
    {                                                           // IsNonZero(x of 8 R): Y holds the prefix, M the value (1 in the place of 0)
        const bool nz = !Fr::is_zero(Fr::canon(p.c[0]));
        const fe x8 = nz ? p.c[0] : Fr::one();
        val[3 * DBL_VARS] = run; val[3 * DBL_VARS + 1] = x8;
        run = Fr::lmul(run, x8);
    }
    const fe *e = fbtab + 3 * (size_t)(int_bit(sw, 0) | (int_bit(sw, 1) << 1));   // fixed base: window i adds entry (s >> 2 i) & 3 of its row
    row[C.window_var0] = e[0]; row[C.window_var0 + 1] = e[1];
    from_affine(p, e[0], e[1]);
#pragma clang loop unroll(disable)
    for (uint32_t i = 1; i < FB_WINDOWS; i++) {
        e = fbtab + 3 * ((size_t)4 * i + (int_bit(sw, 2 * i) | (int_bit(sw, 2 * i + 1) << 1)));
        row[C.window_var0 + 2 * i] = e[0]; row[C.window_var0 + 2 * i + 1] = e[1];
        jj_add(p, e, true);
        park_point(row + C.fixed_adder_var0 + ADD_VARS * (size_t)(i - 1), ADD_VARS, p, run);
    }
}
// the way back over the fixed segment: the fixed-base adders, 1 / x of 8 R, the validator's doublings
ZK_HD void fixed_back(fe *row, const ChainLayout &C, fe &inv) {
    fe *val = row + C.validator_var0;
#pragma clang loop unroll(disable)
    for (uint32_t i = FB_WINDOWS - 1; i >= 1; i--) unpark_point(row + C.fixed_adder_var0 + ADD_VARS * (size_t)(i - 1), ADD_VARS, inv);
    {
        fe *blk8 = val + 2 * DBL_VARS;                          // still projective: X, Y at [4], [5], Z at [0]
        const bool nz = !Fr::is_zero(Fr::canon(blk8[4]));
        const fe xi = Fr::lmul(inv, val[3 * DBL_VARS]);         // 1 / X (or 1 / 1)
        inv = Fr::lmul(inv, val[3 * DBL_VARS + 1]);
        val[3 * DBL_VARS] = bit_fe(nz);
        val[3 * DBL_VARS + 1] = nz ? Fr::canon(Fr::lmul(blk8[0], xi)) : Fr::zero();   // 1 / x = Z / X
    }
#pragma clang loop unroll(disable)
    for (int j = 2; j >= 0; j--) unpark_point(val + DBL_VARS * j, DBL_VARS, inv);
}

// variable base: D = 2^i A, S += bit_i of t ? D : identity (the same instructions either way).  var_start: step 0, D = A and S = the first
// conditional point; var_forward: the steps first .. last (first >= 1), so a caller may restart `run` between two ranges; var_close: rhs = R + t A
ZK_HD void var_start(fe *row, const ChainLayout &C, const fe &ax, const fe &ay, const uint32_t *t, jpoint &d, jpoint &p) {
    from_affine(d, ax, ay);
    const uint32_t b0 = int_bit(t, 0);
    row[C.cond0_var] = b0 ? ax : Fr::zero(); row[C.cond0_var + 1] = b0 ? ay : Fr::one();
    from_affine(p, row[C.cond0_var], row[C.cond0_var + 1]);
}
ZK_HD void var_forward(fe *row, const ChainLayout &C, const uint32_t *t, uint32_t first, uint32_t last, jpoint &d, jpoint &p, fe &run) {
#pragma clang loop unroll(disable)
    for (uint32_t i = first; i <= last; i++) {
        const size_t off = (size_t)(i - 1) * C.step_stride;
        jj_dbl(d, true);
        park_point(row + C.doubler_var0 + off, DBL_VARS, d, run);
        const bool b = int_bit(t, i);
        fe q[4];
        q[0] = b ? d.c[0] : Fr::zero(); q[1] = b ? d.c[1] : Fr::one(); q[2] = b ? jj_mul(coef_d(), d.c[2]) : Fr::zero(); q[3] = b ? d.c[3] : Fr::one();
        jj_add(p, q, false);
        park_point(row + C.adder_var0 + off, ADD_VARS, p, run);
    }
}
ZK_HD void var_close(fe *row, const ChainLayout &C, const fe &rx, const fe &ry, jpoint &p, fe &run) {
    fe q[3];
    q[0] = rx; q[1] = ry; q[2] = jj_mul(coef_d(), jj_mul(rx, ry));
    jj_add(p, q, true);
    park_point(row + C.last_adder_var0, ADD_VARS, p, run);
}
// the way back over the steps first .. last (first >= 1) of the variable-base chains, behind the closing adder where the range holds it
ZK_HD void var_back(fe *row, const ChainLayout &C, uint32_t first, uint32_t last, bool closing, fe &inv) {
    if (closing) unpark_point(row + C.last_adder_var0, ADD_VARS, inv);
#pragma clang loop unroll(disable)
    for (uint32_t i = last; i >= first; i--) {
        const size_t off = (size_t)(i - 1) * C.step_stride;
        unpark_point(row + C.adder_var0 + off, ADD_VARS, inv);
        unpark_point(row + C.doubler_var0 + off, DBL_VARS, inv);
    }
}

// ---- the products of affine inputs, once every x3, y3 is affine.  The validator's three doublers and NotLowOrder's x x, y y
ZK_HD void fill_validator_products(fe *row, const ChainLayout &C, const fe &rx, const fe &ry) {
    fe *val = row + C.validator_var0;
    fill_doubler(val, rx, ry);
    fill_doubler(val + DBL_VARS, val[4], val[5]);
    fill_doubler(val + 2 * DBL_VARS, val[DBL_VARS + 4], val[DBL_VARS + 5]);
    val[3 * DBL_VARS + 2] = Fr::canon(jj_mul(rx, rx)); val[3 * DBL_VARS + 3] = Fr::canon(jj_mul(ry, ry));
}
// the fixed-base adders begin .. end - 1 of 0 .. FB_WINDOWS - 2.  adder i: (window 0 | the previous sum) + window i + 1
ZK_HD void fill_fixed_products(fe *row, const ChainLayout &C, uint32_t begin, uint32_t end) {
#pragma clang loop unroll(disable)
    for (uint32_t i = begin; i < end; i++) {
        fe *blk = row + C.fixed_adder_var0 + ADD_VARS * (size_t)i;
        const fe *prev = i ? blk - 2 : row + C.window_var0, *w = row + C.window_var0 + 2 * (size_t)(i + 1);
        fill_adder(blk, prev[0], prev[1], w[0], w[1]);
    }
}
// the steps begin .. end - 1 of 1 .. N_STEPS: doubler, conditional point, adder; each takes its inputs from the step before (step 1: A, cond0)
ZK_HD void fill_step_products(fe *row, const ChainLayout &C, const uint32_t *t, uint32_t begin, uint32_t end) {
#pragma clang loop unroll(disable)
    for (uint32_t i = begin; i < end; i++) {
        const size_t off = (size_t)(i - 1) * C.step_stride;
        fe *dbl = row + C.doubler_var0 + off, *cond = row + C.cond_var0 + off, *add = row + C.adder_var0 + off;
        const fe *dprev = i > 1 ? dbl - C.step_stride + (DBL_VARS - 2) : row + C.ax_var;
        const fe *sprev = i > 1 ? add - C.step_stride + (ADD_VARS - 2) : row + C.cond0_var;
        fill_doubler(dbl, dprev[0], dprev[1]);
        const bool b = int_bit(t, i);
        cond[0] = b ? dbl[4] : Fr::zero(); cond[1] = b ? dbl[5] : Fr::one();
        fill_adder(add, sprev[0], sprev[1], cond[0], cond[1]);
    }
}
// the closing adder R + (t A) and the verdict: lhs = s B, the last fixed-base sum, == rhs
ZK_HD uint8_t fill_closing(fe *row, const ChainLayout &C, const fe &rx, const fe &ry) {
    const fe *sprev = row + C.adder_var0 + (size_t)(N_STEPS - 1) * C.step_stride + (ADD_VARS - 2);
    fill_adder(row + C.last_adder_var0, rx, ry, sprev[0], sprev[1]);
    const fe *lhs = row + C.fixed_adder_var0 + ADD_VARS * (size_t)(FB_WINDOWS - 2) + ADD_VARS - 2, *rhs = row + C.last_adder_var0 + ADD_VARS - 2;
    return Fr::eq(lhs[0], rhs[0]) && Fr::eq(lhs[1], rhs[1]) ? 1 : 0;
}
// all of them on one lane; returns the verdict
ZK_HD uint8_t fill_all_products(fe *row, const ChainLayout &C, const fe &rx, const fe &ry, const uint32_t *t) {
    fill_validator_products(row, C, rx, ry);
    fill_fixed_products(row, C, 0, FB_WINDOWS - 1);
    fill_step_products(row, C, t, 1, N_STEPS + 1);
    return fill_closing(row, C, rx, ry);
}

// the MiMC hash of R, A and the item's message elements msg, its rounds stored: iv, outputs[i] = key + E_key(x_i) + key + x_i.  Returns t, the
// canonical integer: its bits are the canonical decomposition
ZK_HD fe fill_mimc_hash(fe *row, const FillLayout &L, const fe *__restrict__ rc, const fe *__restrict__ msg, const fe &ax, const fe &ay, const fe &rx, const fe &ry) {
    const uint32_t n_hash = 4 + L.msg_len;
    row[L.iv_var] = Fr::zero();
    fe k = Fr::zero();
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < n_hash; i++) {
        fe xi;
        if (i < 4) xi = i == 0 ? rx : i == 1 ? ry : i == 2 ? ax : ay;
        else { xi = Fr::canon(jj_to_mont(msg[i - 4])); row[L.msg_var0 + (i - 4)] = xi; }
        const fe e = mimc_cipher_rounds(rc, xi, k, row + L.mimc_var0 + n_hash + (size_t)i * MIMC_ROUND_VARS);
        k = Fr::ladd(Fr::ladd(k, xi), e);
        row[L.mimc_var0 + i] = Fr::canon(k);
    }
    return jj_from_mont(k);
}

// fbtab as fixed_forward takes it.  s: any 256-bit integer.  A or R off the curve or s >= 2^254: verdict 0 and the row is not touched.
// Otherwise the whole row, and verdict = (lhs == rhs)
__global__ void __launch_bounds__(BLOCK)
k_eddsa_fill(EddsaView v, const fe *__restrict__ fbtab, FillLayout L, const fe *__restrict__ A, const fe *__restrict__ R, const fe *__restrict__ s,
             const fe *__restrict__ msgs, uint32_t n, fe *d_w, uint64_t row_elems, uint8_t *__restrict__ verdicts) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe ax, ay, rx, ry;
    if (!fill_load_item(A, R, s, g, ax, ay, rx, ry)) { verdicts[g] = 0; return; }
    const uint32_t *__restrict__ sw = s[g].l;
    fe *row = d_w + (size_t)g * row_elems;
    const ChainLayout C = chain_layout(L);

    fill_inputs(row, C, ax, ay, rx, ry, sw);
    const fe t = fill_mimc_hash(row, L, v.rc, msgs + (size_t)g * L.msg_len, ax, ay, rx, ry);
    fill_strict_bits(row + L.t_bit0, row + L.t_range_var0, t.l);

    // ---- the chains, projective, on one running product
    fe run = Fr::one();
    jpoint d, p;
    fixed_forward(row, C, fbtab, rx, ry, sw, run);
    var_start(row, C, ax, ay, t.l, d, p);
    var_forward(row, C, t.l, 1, N_STEPS, d, p, run);
    var_close(row, C, rx, ry, p, run);

    // ---- one inversion, then the way back
    fe inv = jj_inv(run);
    var_back(row, C, 1, N_STEPS, true, inv);
    fixed_back(row, C, inv);

    verdicts[g] = fill_all_products(row, C, rx, ry, t.l);
}

// ---- k_eddsa_fill with ROLES = 2 or 4 lanes per witness: the same row, byte for byte, off a shorter dependent chain.
//
// Roles are WAVE-UNIFORM.  A workgroup is ROLES waves; witness blockIdx.x * 64 + (threadIdx.x & 63) is served by lane (threadIdx.x & 63) of every
// wave, and the wave number threadIdx.x >> 6 is the role, so a branch on the role never splits a wave.  Three phases, two barriers:
//   forward   role 0: the message elements, MiMC with its iv, t with its bits and range products, then both variable-base chains and
//             R + t A, parked as k_eddsa_fill parks them; role 1: the other inputs, the bits of s, the validator, the x of 8 R and the fixed-base chain.  The 637
//             parked items form NSEG segments (WideCut) with a running product each: role 1's 130 items are segment 0, role 0 restarts its
//             running product after the steps var_end(k).  Every segment's total, and t, go to LDS.  Further roles idle here.
//   way back  every role multiplies the totals and inverts the product itself (381 products on all waves at once instead of a third barrier and
//             a broadcast), takes inverse x the OTHER totals as the inverse of a segment it owns, and unparks that segment.
//   gadgets   the products of affine inputs, split evenly by adder and step index; role ROLES - 1 adds the validator's, role 0 the closing
//             adder's and the verdict.
// LDS: (NSEG + 1) slots of 64 x 32 B, each written once before the first barrier and read after it; nothing in LDS is written twice.
//
// Why __syncthreads() alone orders the ROWS, which are global memory written by one wave and read by another on either side of a barrier: a
// workgroup runs on ONE compute unit, whose waves share that unit's one vector L1 (write-through); only workgroups on different units need
// agent-scope release and acquire (workgroup scope does not reach another unit, and need not here).  __syncthreads() is a workgroup-scope
// release fence, s_barrier, and a workgroup-scope acquire fence: the compiler moves no load or store of the rows across it.  For gfx950 it emits
// s_waitcnt lgkmcnt(0) (LDS) and s_barrier with NO vmcnt wait, which is the AMDGPU memory model for this family outside threadgroup-split mode:
// the vector memory requests of all waves of a unit enter its one L1 in issue order, so a store issued before the barrier is ahead of any load
// another wave issues behind it, and needs no completion wait to be seen.  k_mimc_merkle_tail (merkle.hpp) hands tree levels from wave to wave
// the same way.  Every access to a row is a per-lane vector load or store through the non-restrict d_w: nothing of a row goes through the
// scalar cache, which that argument does not cover.
//
// No lane returns before the last barrier: `live` (in range, A and R on the curve, s < 2^254 -- computed by every role for itself) guards every
// load and store of a witness, the barriers stand outside it.  A malformed item: verdict 0 from role 0, the row untouched by every role.
template <uint32_t ROLES> struct WideCut {
    static constexpr uint32_t NV = ROLES == 4 ? 3 : 2, NSEG = NV + 1;   // segment 0: validator, x of 8 R, fixed base; 1 + k: the steps up to var_end(k)
    // the last step of variable segment k (the last segment also holds the closing adder).  4 roles: 129 + 1 | 168 | 170 | 169 items, one segment
    // a role; 2 roles: role 1 owns 129 + 1 and 188, role 0 owns 319
    ZK_HD static constexpr uint32_t var_end(uint32_t k) { return ROLES == 4 ? (k == 0 ? 84 : k == 1 ? 169 : N_STEPS) : (k == 0 ? 94 : N_STEPS); }
    ZK_HD static constexpr uint32_t owner(uint32_t sg) { return ROLES == 4 ? (sg == 0 ? 1 : sg == 1 ? 0 : sg) : (sg == 2 ? 0 : 1); }
};

// arguments, malformed items, verdicts and the row as k_eddsa_fill; launched with zk_div_up(n, 64) workgroups of 64 ROLES threads
template <uint32_t ROLES>
__global__ void __launch_bounds__(BLOCK * ROLES)
k_eddsa_fill_wide(EddsaView v, const fe *__restrict__ fbtab, FillLayout L, const fe *__restrict__ A, const fe *__restrict__ R, const fe *__restrict__ s,
                  const fe *__restrict__ msgs, uint32_t n, fe *d_w, uint64_t row_elems, uint8_t *__restrict__ verdicts) {
    using Cut = WideCut<ROLES>;
    constexpr uint32_t NSEG = Cut::NSEG, T_SLOT = NSEG;
    __shared__ fe xch[NSEG + 1][BLOCK];                         // the segments' totals and t, per witness of the workgroup
    const uint32_t j = threadIdx.x & (BLOCK - 1), role = threadIdx.x / BLOCK;
    const uint32_t g = blockIdx.x * BLOCK + j;
    const bool in_range = g < n;
    const size_t gi = in_range ? g : 0;                         // a lane out of range forms no address past the arrays
    const uint32_t *__restrict__ sw = s[gi].l;
    fe ax = Fr::zero(), ay = ax, rx = ax, ry = ax;
    const bool live = in_range && fill_load_item(A, R, s, gi, ax, ay, rx, ry);
    fe *row = d_w + gi * row_elems;
    const ChainLayout C = chain_layout(L);

    // ---- forward
    if (live && role == 0) {
        // the hash is fill_mimc_hash written out.  Called as that function the loop's temporaries share a stack slot and the kernel's scratch
        // falls from 1 088 to 1 056 B a lane, a wave's from 17 to 16.5 pages of 4 KiB -- and at 2^14 witnesses, a workgroup on every compute
        // unit, the kernel is 1 % slower for it (profiles/eddsa_fill_refactor_ab.txt).  k_eddsa_fill, a quarter of the waves, does not notice
        const uint32_t n_hash = 4 + L.msg_len;
        row[L.iv_var] = Fr::zero();
        fe k = Fr::zero();
#pragma clang loop unroll(disable)
        for (uint32_t i = 0; i < n_hash; i++) {
            fe xi;
            if (i < 4) xi = i == 0 ? rx : i == 1 ? ry : i == 2 ? ax : ay;
            else { xi = Fr::canon(jj_to_mont(msgs[gi * L.msg_len + (i - 4)])); row[L.msg_var0 + (i - 4)] = xi; }
            const fe e = mimc_cipher_rounds(v.rc, xi, k, row + L.mimc_var0 + n_hash + (size_t)i * MIMC_ROUND_VARS);
            k = Fr::ladd(Fr::ladd(k, xi), e);
            row[L.mimc_var0 + i] = Fr::canon(k);
        }
        const fe t = jj_from_mont(k);
        xch[T_SLOT][j] = t;
        fill_strict_bits(row + L.t_bit0, row + L.t_range_var0, t.l);
        fe run = Fr::one();
        jpoint d, p;
        var_start(row, C, ax, ay, t.l, d, p);
#pragma clang loop unroll(disable)
        for (uint32_t k = 0; k < Cut::NV; k++) {                // a segment ends: its total, a new product
            var_forward(row, C, t.l, k ? Cut::var_end(k - 1) + 1 : 1, Cut::var_end(k), d, p, run);
            if (k + 1 == Cut::NV) var_close(row, C, rx, ry, p, run);
            xch[1 + k][j] = run;
            run = Fr::one();
        }
    } else if (live && role == 1) {
        fill_inputs(row, C, ax, ay, rx, ry, sw);
        fe run = Fr::one();
        fixed_forward(row, C, fbtab, rx, ry, sw, run);
        xch[0][j] = run;
    }
    __syncthreads();

    // ---- one inversion on every role, then each role's own segments on the way back
    fe t = Fr::zero();
    if (live) {
        t = xch[T_SLOT][j];
        fe tot[NSEG];
        for (uint32_t k = 0; k < NSEG; k++) tot[k] = xch[k][j];
        fe all = tot[0];
        for (uint32_t k = 1; k < NSEG; k++) all = jj_mul(all, tot[k]);
        const fe inv_all = jj_inv(all);
        for (uint32_t sg = 0; sg < NSEG; sg++) {
            if (Cut::owner(sg) != role) continue;
            fe inv = inv_all;                                   // 1 / (this segment's total) = 1 / (all) x the other totals
            for (uint32_t k = 0; k < NSEG; k++) if (k != sg) inv = jj_mul(inv, tot[k]);
            if (sg == 0) fixed_back(row, C, inv);
            else var_back(row, C, sg == 1 ? 1 : Cut::var_end(sg - 2) + 1, Cut::var_end(sg - 1), sg == Cut::NV, inv);
        }
    }
    __syncthreads();

    // ---- the products of affine inputs: an even share of the fixed-base adders and of the steps on every role
    if (live) {
        fill_fixed_products(row, C, (FB_WINDOWS - 1) * role / ROLES, (FB_WINDOWS - 1) * (role + 1) / ROLES);
        fill_step_products(row, C, t.l, 1 + N_STEPS * role / ROLES, 1 + N_STEPS * (role + 1) / ROLES);
        if (role == ROLES - 1) fill_validator_products(row, C, rx, ry);
    }
    if (role == 0 && in_range) verdicts[g] = live ? fill_closing(row, C, rx, ry) : 0;   // the one role that answers
}

// ---- the complete witness of the PureEdDSA circuit (jubjub_gadgets.py, eddsa_pure_circuit): the row of the MiMC-EdDSA circuit with the
// windowed Pedersen hash in the place of MiMC.  PureLayout is zk_eddsa_pure_layout of zkhip.h; the host has checked it as it checks FillLayout.
//
// TWO inversions per witness, whatever the number of windows.  The hash names, per window past the first of a segment, the AFFINE MONTGOMERY
// running sum (X3, Y3 of a MontgomeryAdder) and the slope lambda = (v2 - v1) / (u2 - u1) that led to it, and per segment the affine Edwards sum
// (MontgomeryToEdwards).  The lane walks a segment's running sum in extended Edwards coordinates with the mixed additions of k_jj_pedersen and
// takes every quotient from (X : Y : Z):  u = (Z + Y) / (Z - Y),  v = u Z / X,  u2 - u = (u2 (Z - Y) - (Z + Y)) / (Z - Y), u2 the tabulated
// Montgomery x of the next window's table point.  One denominator a step, E = (Z - Y) X D3 with D3 = u2 (Z - Y) - (Z + Y) -- or Z at the end of a
// segment, where 1 / Z gives the converter's Edwards point -- joins the running product of the chains: 1 / (Z - Y) = X D3 / E,
// 1 / ((Z - Y) X) = D3 / E, 1 / D3 = (Z - Y) X / E.  (X, Y, Z) wait in the adder's three slots, the prefix product and E in the window's two.
// The first window of a segment is a table point: its step's denominator is u2 - u0, two table values.  No step has a special case (the argument
// is at FixedBaseMulZcash in jubjub_gadgets.py and in DESIGN 5k).  The first inversion closes the validator, the fixed-base chain and the hash
// and yields t; the second closes the variable-base chain, which needs the bits of t.
struct PureLayout {
    uint32_t msg_len, n_vars, ax_var, msg_bit0, rx_var, s_bit0, pad_bit0, validator_var0, window_var0, fixed_adder_var0, rx_bit0, rx_range_var0,
             ax_bit0, ax_range_var0, hash_window_var0, mont_adder_var0, converter_var0, edwards_adder_var0, t_bit0, t_range_var0, cond0_var,
             doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0;
};
constexpr uint32_t MADD_VARS = 3, SEG_ADDERS = SEG_WINDOWS - 1;
ZK_HD uint32_t pure_windows(uint32_t msg_len) { return (2 * FIELD_BITS + 8 * msg_len + 2) / 3; }

// one in-circuit hash: tab / mtab = its table and, per entry of it, the Montgomery form (u, v) = ((1 + y) / (1 - y), u / x) of the table point,
// canonical Montgomery; hw, madd, conv, ed = its windows, Montgomery adders, converters and Edwards adders in the row; W windows over the bits
// of the stream from bit0 on
struct HashWalk {
    const fe *tab, *mtab;
    fe *hw, *madd, *conv, *ed;
    uint32_t W, bit0;
    ZK_HD uint32_t lone() const { return W % SEG_WINDOWS == 1 ? 1u : 0u; }
    ZK_HD uint32_t n_seg() const { return (W - lone() + SEG_WINDOWS - 1) / SEG_WINDOWS; }
    ZK_HD uint32_t seg_windows(uint32_t sg) const { const uint32_t left = W - lone() - sg * SEG_WINDOWS; return left < SEG_WINDOWS ? left : SEG_WINDOWS; }   // >= 2
    ZK_HD uint32_t window(const BitStream &bs, uint32_t j) const { const uint32_t i = bit0 + 3 * j; return bs.bit(i) | (bs.bit(i + 1) << 1) | (bs.bit(i + 2) << 2); }
};

// the forward walk of one hash: per window the prefix product and the denominator E wait in the window's two slots, (X, Y, Z) in the adder's
// three; the Edwards sums of the segments are parked like every other point
ZK_HD void hash_walk_forward(const HashWalk &h, const BitStream &bs, fe &run) {
    const uint32_t W = h.W, lone = h.lone(), n_seg = h.n_seg();
    jpoint hacc, p;
    if (lone) {                                                 // the last base point's single window: its converter is the table point itself
        const uint32_t j = W - 1, w = h.window(bs, j);
        const fe *e = h.tab + ((size_t)j * 4 + (w & 3)) * 3;
        const fe x = Fr::canon(neg_if(e[0], w > 3));
        h.conv[0] = x; h.conv[1] = e[1];
        from_affine(hacc, x, e[1]);
    }
#pragma clang loop unroll(disable)
    for (uint32_t sg = 0; sg < n_seg; sg++) {
        const uint32_t j0 = sg * SEG_WINDOWS, m = h.seg_windows(sg);
        uint32_t w = h.window(bs, j0);
        {
            const fe *e = h.tab + ((size_t)j0 * 4 + (w & 3)) * 3;
            from_affine(p, neg_if(e[0], w > 3), e[1]);
        }
#pragma clang loop unroll(disable)
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t j = j0 + k;
            const bool last = k + 1 == m;
            const uint32_t w2 = last ? 0u : h.window(bs, j + 1);
            const fe u2 = h.mtab[((size_t)(last ? j : j + 1) * 4 + (w2 & 3)) * 2];
            fe E;
            if (k == 0) E = Fr::lsub(u2, h.mtab[((size_t)j * 4 + (w & 3)) * 2]);
            else {
                fe *blk = h.madd + MADD_VARS * (size_t)(sg * SEG_ADDERS + k - 1);
                blk[0] = p.c[0]; blk[1] = p.c[1]; blk[2] = p.c[3];
                const fe d1 = Fr::lsub(p.c[3], p.c[1]);
                const fe d3 = last ? p.c[3] : Fr::lsub(Fr::lmul(u2, d1), Fr::ladd(p.c[3], p.c[1]));
                E = Fr::lmul(Fr::lmul(d1, p.c[0]), d3);
            }
            h.hw[2 * (size_t)j] = run; h.hw[2 * (size_t)j + 1] = E;
            run = Fr::lmul(run, E);
            if (!last) { pedersen_step(p, h.tab, j + 1, w2); w = w2; }
        }
        if (!lone && sg == 0) hacc = p;
        else {
            fe q[4];
            q[0] = p.c[0]; q[1] = p.c[1]; q[2] = jj_mul(coef_d(), p.c[2]); q[3] = p.c[3];
            jj_add(hacc, q, false);
            park_point(h.ed + ADD_VARS * (size_t)(sg - 1 + lone), ADD_VARS, hacc, run);
        }
    }
}

// the way back: inv = 1 / (the product up to and including the hash's last denominator) on entry, 1 / (the product before its first) on return.
// Leaves every window, Montgomery adder and converter of the hash as the front end has it, and x3, y3 of every Edwards adder
ZK_HD void hash_walk_back(const HashWalk &h, const BitStream &bs, fe &inv) {
    const uint32_t W = h.W, lone = h.lone(), n_seg = h.n_seg();
#pragma clang loop unroll(disable)
    for (int sg = (int)n_seg - 1; sg >= 0; sg--) {
        const uint32_t j0 = sg * SEG_WINDOWS, m = h.seg_windows(sg);
        if (lone || sg > 0) unpark_point(h.ed + ADD_VARS * (size_t)(sg - 1 + lone), ADD_VARS, inv);
#pragma clang loop unroll(disable)
        for (int k = (int)m - 1; k >= 0; k--) {
            const uint32_t j = j0 + k;
            const bool last = k + 1 == (int)m;
            fe *win = h.hw + 2 * (size_t)j;
            const fe einv = Fr::lmul(inv, win[0]);              // 1 / E of this step
            inv = Fr::lmul(inv, win[1]);
            const uint32_t w = h.window(bs, j), w2 = last ? 0u : h.window(bs, j + 1);
            const fe vown = Fr::canon(neg_if(h.mtab[((size_t)j * 4 + (w & 3)) * 2 + 1], w > 3));
            const fe *m2 = h.mtab + ((size_t)(last ? j : j + 1) * 4 + (w2 & 3)) * 2;
            const fe u2 = m2[0], v2 = neg_if(m2[1], w2 > 3);
            if (k == 0) h.madd[MADD_VARS * (size_t)(sg * SEG_ADDERS)] = Fr::canon(Fr::lmul(Fr::lsub(v2, vown), einv));
            else {
                fe *blk = h.madd + MADD_VARS * (size_t)(sg * SEG_ADDERS + k - 1);
                const fe X = blk[0], Y = blk[1], Z = blk[2];
                const fe d1 = Fr::lsub(Z, Y), zpy = Fr::ladd(Z, Y);
                const fe d3 = last ? Z : Fr::lsub(Fr::lmul(u2, d1), zpy);
                const fe i2 = Fr::lmul(einv, d3), i1 = Fr::lmul(i2, X);                  // 1 / ((Z - Y) X), 1 / (Z - Y)
                const fe i3 = Fr::lmul(einv, Fr::lmul(d1, X));                            // 1 / D3
                const fe vv = Fr::lmul(Fr::lmul(zpy, Z), i2);
                blk[1] = Fr::canon(Fr::lmul(zpy, i1)); blk[2] = Fr::canon(vv);
                if (last) {
                    fe *c = h.conv + 2 * (size_t)(sg + lone);
                    c[0] = Fr::canon(Fr::lmul(X, i3)); c[1] = Fr::canon(Fr::lmul(Y, i3));
                } else blk[MADD_VARS] = Fr::canon(Fr::lmul(Fr::lsub(v2, vv), Fr::lmul(i3, d1)));   // the next adder's lambda
            }
            win[0] = bit_fe((w & 3) == 3); win[1] = vown;
        }
    }
    if (lone) {
        const uint32_t j = W - 1, w = h.window(bs, j);
        h.hw[2 * (size_t)j] = bit_fe((w & 3) == 3);
        h.hw[2 * (size_t)j + 1] = Fr::canon(neg_if(h.mtab[((size_t)j * 4 + (w & 3)) * 2 + 1], w > 3));
    }
}

// the products of the Edwards adders over the converted segments; returns the x of the hash (canonical Montgomery): the last adder's, or the
// only converter's when the hash has one segment (the message hash of a short message; the hash over R, A, M always has three or more)
ZK_HD fe hash_walk_close(const HashWalk &h) {
    const uint32_t n_conv = h.n_seg() + h.lone();
    const fe *prev = h.conv;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i + 1 < n_conv; i++) {
        fe *blk = h.ed + ADD_VARS * (size_t)i;
        fill_adder(blk, prev[0], prev[1], h.conv[2 * (size_t)(i + 1)], h.conv[2 * (size_t)(i + 1) + 1]);
        prev = blk + ADD_VARS - 2;
    }
    return prev[0];
}

// mtab: the (u, v) of every entry of ram_tab, as HashWalk takes it.  msgs: msg_len bytes an item.  Malformed items, verdicts and the row's form
// as k_eddsa_fill
__global__ void __launch_bounds__(BLOCK)
k_eddsa_fill_pure(EddsaView v, const fe *__restrict__ fbtab, const fe *__restrict__ mtab, PureLayout L, const fe *__restrict__ A, const fe *__restrict__ R,
                  const fe *__restrict__ s, const uint8_t *__restrict__ msgs, uint32_t n, fe *d_w, uint64_t row_elems, uint8_t *__restrict__ verdicts) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe ax, ay, rx, ry;
    if (!fill_load_item(A, R, s, g, ax, ay, rx, ry)) { verdicts[g] = 0; return; }
    const uint32_t *__restrict__ sw = s[g].l;
    fe *row = d_w + (size_t)g * row_elems;
    const ChainLayout C = chain_layout(L);
    BitStream bs;
    bs.rx = R[2 * (size_t)g].l; bs.ax = A[2 * (size_t)g].l; bs.mx = nullptr; bs.msg = msgs + (size_t)g * L.msg_len; bs.msg_bits = 8 * L.msg_len;
    HashWalk h;                                                 // the whole stream: bits(R.x) || bits(A.x) || the message bits
    h.tab = v.ram_tab; h.mtab = mtab; h.W = v.ram_windows; h.bit0 = 0;
    h.hw = row + L.hash_window_var0; h.madd = row + L.mont_adder_var0; h.conv = row + L.converter_var0; h.ed = row + L.edwards_adder_var0;

    // ---- the inputs and the two decompositions that feed the hash
    fill_inputs(row, C, ax, ay, rx, ry, sw);
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < bs.msg_bits; i++) row[L.msg_bit0 + i] = bit_fe(bs.bit(2 * FIELD_BITS + i));
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < 3 * h.W - 2 * FIELD_BITS - bs.msg_bits; i++) row[L.pad_bit0 + i] = Fr::zero();
    fill_strict_bits(row + L.rx_bit0, row + L.rx_range_var0, bs.rx);
    fill_strict_bits(row + L.ax_bit0, row + L.ax_range_var0, bs.ax);

    // ---- the first set of chains, projective: validator, fixed base, hash; the first inversion and its way back; t = the hash's x, its bits
    fe run = Fr::one();
    fixed_forward(row, C, fbtab, rx, ry, sw, run);
    hash_walk_forward(h, bs, run);
    fe inv = jj_inv(run);
    hash_walk_back(h, bs, inv);
    fixed_back(row, C, inv);
    const fe t = jj_from_mont(hash_walk_close(h));
    fill_strict_bits(row + L.t_bit0, row + L.t_range_var0, t.l);

    // ---- the second set: variable base and R + t A
    run = Fr::one();
    jpoint d, p;
    var_start(row, C, ax, ay, t.l, d, p);
    var_forward(row, C, t.l, 1, N_STEPS, d, p, run);
    var_close(row, C, rx, ry, p, run);
    inv = jj_inv(run);
    var_back(row, C, 1, N_STEPS, true, inv);

    verdicts[g] = fill_all_products(row, C, rx, ry, t.l);
}

// ---- the complete witness of the EdDSA circuit of the "hash" scheme (jubjub_gadgets.py, EddsaHashCircuit): the row of k_eddsa_fill_pure with a
// SECOND in-circuit Pedersen hash in front, M = the hash "EdDSA_Verify.M" of the message bits, whose 254 strict bits are the third part of the
// input of the hash "EdDSA_Verify.RAM".  HashLayout is zk_eddsa_hash_layout of zkhip.h; the host has checked it as it checks PureLayout.
//
// THREE inversions per witness, whatever msg_len.  The message hash joins the product of the validator and of the fixed-base chain, which need
// nothing from it: the first inversion closes all three and yields M.x.  The RAM hash needs the bits of M.x and yields t (the second
// inversion); the variable-base chain needs the bits of t (the third).  The message hash may have a single segment (msg_len <= 23: no Edwards
// adder, M is the converter's point) and, unlike the RAM hash of this circuit, a lone last window (W_m % 62 == 1).  No step has a special case:
// DESIGN 5m restates the argument of 5k for the table of "EdDSA_Verify.M".
struct HashLayout {
    uint32_t msg_len, n_vars, ax_var, msg_bit0, rx_var, s_bit0, validator_var0, window_var0, fixed_adder_var0, rx_bit0, rx_range_var0,
             ax_bit0, ax_range_var0, hash_window_var0, mont_adder_var0, converter_var0, edwards_adder_var0, t_bit0, t_range_var0, cond0_var,
             doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0, m_pad_bit0, m_window_var0, m_mont_adder_var0, m_converter_var0,
             m_edwards_adder_var0, m_bit0, m_range_var0;
};
constexpr uint32_t HASH_RAM_WINDOWS = FIELD_BITS;                // 3 x 254 bits: 254 windows, segments of 62, 62, 62, 62 and 6
ZK_HD uint32_t hash_msg_windows(uint32_t msg_len) { return (8 * msg_len + 2) / 3; }

// mtab / m_mtab: the (u, v) of every entry of ram_tab / m_tab.  msgs: msg_len bytes an item.  Malformed items, verdicts and the row's form as
// k_eddsa_fill
__global__ void __launch_bounds__(BLOCK)
k_eddsa_fill_hash(EddsaView v, const fe *__restrict__ fbtab, const fe *__restrict__ mtab, const fe *__restrict__ m_mtab, HashLayout L, const fe *__restrict__ A,
                  const fe *__restrict__ R, const fe *__restrict__ s, const uint8_t *__restrict__ msgs, uint32_t n, fe *d_w, uint64_t row_elems,
                  uint8_t *__restrict__ verdicts) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    fe ax, ay, rx, ry;
    if (!fill_load_item(A, R, s, g, ax, ay, rx, ry)) { verdicts[g] = 0; return; }
    const uint32_t *__restrict__ sw = s[g].l;
    fe *row = d_w + (size_t)g * row_elems;
    const ChainLayout C = chain_layout(L);
    BitStream bs;
    bs.rx = R[2 * (size_t)g].l; bs.ax = A[2 * (size_t)g].l; bs.mx = nullptr; bs.msg = msgs + (size_t)g * L.msg_len; bs.msg_bits = 8 * L.msg_len;
    HashWalk hm, hr;                                            // the message hash reads the stream from the message on (past its end: the zero padding)
    hm.tab = v.m_tab; hm.mtab = m_mtab; hm.W = v.m_windows; hm.bit0 = 2 * FIELD_BITS;
    hm.hw = row + L.m_window_var0; hm.madd = row + L.m_mont_adder_var0; hm.conv = row + L.m_converter_var0; hm.ed = row + L.m_edwards_adder_var0;
    hr.tab = v.ram_tab; hr.mtab = mtab; hr.W = v.ram_windows; hr.bit0 = 0;
    hr.hw = row + L.hash_window_var0; hr.madd = row + L.mont_adder_var0; hr.conv = row + L.converter_var0; hr.ed = row + L.edwards_adder_var0;

    // ---- the inputs and the two decompositions that need nothing else
    fill_inputs(row, C, ax, ay, rx, ry, sw);
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < bs.msg_bits; i++) row[L.msg_bit0 + i] = bit_fe(bs.bit(2 * FIELD_BITS + i));
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < 3 * hm.W - bs.msg_bits; i++) row[L.m_pad_bit0 + i] = Fr::zero();
    fill_strict_bits(row + L.rx_bit0, row + L.rx_range_var0, bs.rx);
    fill_strict_bits(row + L.ax_bit0, row + L.ax_range_var0, bs.ax);

    // ---- the first set of chains, projective: validator, fixed base, the message hash; the first inversion and its way back; M = the message
    // hash, the strict bits of its x
    fe run = Fr::one();
    fixed_forward(row, C, fbtab, rx, ry, sw, run);
    hash_walk_forward(hm, bs, run);
    fe inv = jj_inv(run);
    hash_walk_back(hm, bs, inv);
    fixed_back(row, C, inv);
    const fe mx = jj_from_mont(hash_walk_close(hm));            // the canonical integer: the third part of the RAM hash's input
    fill_strict_bits(row + L.m_bit0, row + L.m_range_var0, mx.l);

    // ---- the RAM hash over bits(R.x) || bits(A.x) || bits(M.x): the second inversion; t = its x, the strict bits of t
    bs.mx = mx.l;
    run = Fr::one();
    hash_walk_forward(hr, bs, run);
    inv = jj_inv(run);
    hash_walk_back(hr, bs, inv);
    const fe t = jj_from_mont(hash_walk_close(hr));
    fill_strict_bits(row + L.t_bit0, row + L.t_range_var0, t.l);

    // ---- the third set: variable base and R + t A
    run = Fr::one();
    jpoint d, p;
    var_start(row, C, ax, ay, t.l, d, p);
    var_forward(row, C, t.l, 1, N_STEPS, d, p, run);
    var_close(row, C, rx, ry, p, run);
    inv = jj_inv(run);
    var_back(row, C, 1, N_STEPS, true, inv);

    verdicts[g] = fill_all_products(row, C, rx, ry, t.l);
}

}  // namespace jubjub
}  // namespace zk
