// pairing.hpp -- the optimal-ate pairing of BN254 for host, device and the CPU emulation (one text, like bn254.hpp).
//
// Tower: Fq2 = Fq[u]/(u^2 + 1) (bn254.hpp), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = 9 + u.  An Fq12 element
// sum a_ij v^i w^j is {c0 = (a00, a10, a20), c1 = (a01, a11, a21)}; in the polynomial basis of verify.cpp / oracle/pyref.py
// (Fq[w]/(w^12 - 18 w^6 + 82)) the coefficient a_ij sits at w^(2i + j) with u = w^6 - 9.
//
// Miller loop: f_{6z+2,Q}(P) l_{.,pi(Q)}(P) l_{.,-pi^2(Q)}(P), z = 4965661367192848881, the bits of 6z + 2 from the top (no NAF:
// 64 doublings, 36 additions, 2 Frobenius steps = MILLER_STEPS lines), T in homogeneous projective coordinates on the twist
// (Costello-Lange-Naehrig): no inversion inside the loop.  A line is the sparse element a y_P + (b x_P) w + c v w; the step
// functions return (a, b, c), which depend on Q alone, so the fixed-Q form (gamma, delta of a key) reads them from a table
// that the variable-Q walk wrote once.  Lines are scaled by elements of Fq2, which the final exponentiation removes.
// A multi-pairing shares the squaring of f.  A pair with P or Q at infinity contributes the factor 1: its lines are
// replaced by 1 through selection, every lane runs the same instructions.  The loop and chain bits are compile-time
// constants (uniform branches).  Points are expected in the order-r groups (the walk has no exceptional cases there); any
// other input gives a defined but meaningless value, never a fault.
//
// Final exponentiation: easy part (q^6 - 1)(q^2 + 1) with one Fq12 inversion (one Fq inversion at the bottom), hard part by
// the addition chain in z of Fuentes-Castaneda, Knapp and Rodriguez-Henriquez (SAC 2011) with Granger-Scott cyclotomic
// squarings.  The chain computes f^(c (q^12 - 1)/r) with c = 2z (6z^2 + 3z + 1), which is coprime to r: the value is only
// ever compared with 1 or with a value made by this same code (e(alpha, beta) of a verifier context).
//
// Arithmetic runs in the loose domain [0, 2q) of bn254.hpp (strict on the host); compare through f12_eq / f12_is_one.
//
// Code size and registers: an Fq12 is 96 VGPRs, so the building blocks are real functions (ZK_PFN: not inlined) that
// work on operands in memory -- on the device the lane's private (scratch) memory -- and only the Fq2 product / square
// hold a full working set in registers.  The whole pairing is a few tens of KB of code instead of megabytes, and the
// scratch traffic per Fq2 product (192 bytes) is small against its ~1500 VALU instructions.
#pragma once
#include "bn254.hpp"
#include "pairing_consts.hpp"

namespace zk {
namespace pairing {

#define ZK_PFN inline ZK_HD_NOINLINE

struct alignas(16) fe6 { fe2 c0, c1, c2; };
struct alignas(16) fe12 { fe6 c0, c1; };
struct alignas(16) G2Hom { fe2 x, y, z; };          // point of the twist, homogeneous projective (z = 0: infinity)
struct alignas(16) LineC { fe2 a, b, c; };          // line coefficients: a y_P + (b x_P) w + c v w

constexpr uint64_t BN_Z = 4965661367192848881ull;
constexpr uint64_t ATE_LOW = 0x9d797039be763ba8ull;  // low 64 bits of 6z + 2 = 0x19d797039be763ba8 (bit 64 is the leading one)
constexpr uint32_t MILLER_STEPS = 64 + 36 + 2;

// ---------------------------------------------------------------- Fq2 helpers
ZK_PFN void f2mul(fe2 &r, const fe2 &a, const fe2 &b) { r = Fq2::lmul(a, b); }
ZK_PFN void f2sqr(fe2 &r, const fe2 &a) { r = Fq2::lsqr(a); }
ZK_PFN void f2muls(fe2 &r, const fe2 &a, const fe &s) { fe2 t; t.c0 = Fq::lmul(a.c0, s); t.c1 = Fq::lmul(a.c1, s); r = t; }
ZK_PFN void f2inv(fe2 &r, const fe2 &a) { r = Fq2::inv(Fq2::canon(a)); }                 // strict; 0 -> 0
ZK_HD fe2 f2add(const fe2 &a, const fe2 &b) { return Fq2::ladd(a, b); }
ZK_HD fe2 f2sub(const fe2 &a, const fe2 &b) { return Fq2::lsub(a, b); }
ZK_HD fe2 f2dbl(const fe2 &a) { return Fq2::ldbl(a); }
ZK_HD fe2 f2neg(const fe2 &a) { return Fq2::lneg(a); }
ZK_HD fe2 f2conj(const fe2 &a) { fe2 r; r.c0 = a.c0; r.c1 = Fq::lneg(a.c1); return r; }
ZK_HD fe2 f2mulxi(const fe2 &a) {                     // (9 + u)(a0 + a1 u) = (9 a0 - a1) + (9 a1 + a0) u
    const fe2 n = Fq2::ladd(Fq2::ldbl(Fq2::ldbl(Fq2::ldbl(a))), a);
    fe2 r; r.c0 = Fq::lsub(n.c0, a.c1); r.c1 = Fq::ladd(n.c1, a.c0); return r;
}
ZK_HD fe fsel(bool c, const fe &a, const fe &b) {     // c ? a : b, limb by limb (no branch)
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
ZK_HD fe2 f2sel(bool c, const fe2 &a, const fe2 &b) { fe2 r; r.c0 = fsel(c, a.c0, b.c0); r.c1 = fsel(c, a.c1, b.c1); return r; }
ZK_HD bool f2eq(const fe2 &a, const fe2 &b) { return Fq2::eq(Fq2::canon(a), Fq2::canon(b)); }

// ---------------------------------------------------------------- Fq6
ZK_HD fe6 f6zero() { fe6 r; r.c0 = Fq2::zero(); r.c1 = Fq2::zero(); r.c2 = Fq2::zero(); return r; }
ZK_HD fe6 f6one() { fe6 r = f6zero(); r.c0 = Fq2::one(); return r; }
ZK_PFN void f6add(fe6 &r, const fe6 &a, const fe6 &b) { r.c0 = f2add(a.c0, b.c0); r.c1 = f2add(a.c1, b.c1); r.c2 = f2add(a.c2, b.c2); }
ZK_PFN void f6sub(fe6 &r, const fe6 &a, const fe6 &b) { r.c0 = f2sub(a.c0, b.c0); r.c1 = f2sub(a.c1, b.c1); r.c2 = f2sub(a.c2, b.c2); }
ZK_PFN void f6neg(fe6 &r, const fe6 &a) { r.c0 = f2neg(a.c0); r.c1 = f2neg(a.c1); r.c2 = f2neg(a.c2); }
ZK_PFN void f6mulv(fe6 &r, const fe6 &a) { const fe2 t = f2mulxi(a.c2); r.c2 = a.c1; r.c1 = a.c0; r.c0 = t; }      // v (c0, c1, c2) = (xi c2, c0, c1)
// Karatsuba (Devegili et al.): 6 Fq2 products
ZK_PFN void f6mul(fe6 &r, const fe6 &a, const fe6 &b) {
    fe2 v0, v1, v2, t0, t1, t2;
    f2mul(v0, a.c0, b.c0); f2mul(v1, a.c1, b.c1); f2mul(v2, a.c2, b.c2);
    f2mul(t0, f2add(a.c1, a.c2), f2add(b.c1, b.c2));
    f2mul(t1, f2add(a.c0, a.c1), f2add(b.c0, b.c1));
    f2mul(t2, f2add(a.c0, a.c2), f2add(b.c0, b.c2));
    r.c0 = f2add(v0, f2mulxi(f2sub(f2sub(t0, v1), v2)));
    r.c1 = f2add(f2sub(f2sub(t1, v0), v1), f2mulxi(v2));
    r.c2 = f2add(f2sub(f2sub(t2, v0), v2), v1);
}
// a (b0 + b1 v): 5 Fq2 products
ZK_PFN void f6mul01(fe6 &r, const fe6 &a, const fe2 &b0, const fe2 &b1) {
    fe2 aa, bb, t1, t2, t3;
    f2mul(aa, a.c0, b0); f2mul(bb, a.c1, b1);
    f2mul(t1, f2add(a.c1, a.c2), b1);
    f2mul(t3, f2add(a.c0, a.c2), b0);
    f2mul(t2, f2add(a.c0, a.c1), f2add(b0, b1));
    r.c0 = f2add(f2mulxi(f2sub(t1, bb)), aa);
    r.c1 = f2sub(f2sub(t2, aa), bb);
    r.c2 = f2add(f2sub(t3, aa), bb);
}
ZK_PFN void f6inv(fe6 &r, const fe6 &a) {
    fe2 t0, t1, t2, s, d;
    f2sqr(t0, a.c0); f2mul(s, a.c1, a.c2); t0 = f2sub(t0, f2mulxi(s));           // c0^2 - xi c1 c2
    f2sqr(t1, a.c2); f2mul(s, a.c0, a.c1); t1 = f2sub(f2mulxi(t1), s);           // xi c2^2 - c0 c1
    f2sqr(t2, a.c1); f2mul(s, a.c0, a.c2); t2 = f2sub(t2, s);                    // c1^2 - c0 c2
    f2mul(d, a.c2, t1); f2mul(s, a.c1, t2); d = f2mulxi(f2add(d, s));
    f2mul(s, a.c0, t0); d = f2add(d, s);
    f2inv(d, d);
    f2mul(r.c0, t0, d); f2mul(r.c1, t1, d); f2mul(r.c2, t2, d);
}

// ---------------------------------------------------------------- Fq12
ZK_HD fe12 f12one() { fe12 r; r.c0 = f6one(); r.c1 = f6zero(); return r; }
ZK_PFN void f12mul(fe12 &r, const fe12 &a, const fe12 &b) {
    fe6 v0, v1, s, t;
    f6mul(v0, a.c0, b.c0); f6mul(v1, a.c1, b.c1);
    f6add(s, a.c0, a.c1); f6add(t, b.c0, b.c1);
    f6mul(s, s, t);
    f6sub(s, s, v0); f6sub(r.c1, s, v1);
    f6mulv(v1, v1); f6add(r.c0, v0, v1);
}
ZK_PFN void f12sqr(fe12 &r, const fe12 &a) {           // complex squaring: 2 Fq6 products
    fe6 ab, s, t;
    f6mul(ab, a.c0, a.c1);
    f6mulv(t, a.c1); f6add(t, t, a.c0);
    f6add(s, a.c0, a.c1);
    f6mul(s, s, t);                                    // (c0 + c1)(c0 + v c1) = c0^2 + v c1^2 + ab + v ab
    f6sub(s, s, ab); f6mulv(t, ab); f6sub(r.c0, s, t);
    f6add(r.c1, ab, ab);
}
ZK_PFN void f12conj(fe12 &r, const fe12 &a) { r.c0 = a.c0; f6neg(r.c1, a.c1); }
ZK_PFN void f12inv(fe12 &r, const fe12 &a) {
    fe6 t0, t1;
    f6mul(t0, a.c0, a.c0); f6mul(t1, a.c1, a.c1);
    f6mulv(t1, t1); f6sub(t0, t0, t1);                 // c0^2 - v c1^2
    f6inv(t0, t0);
    f6mul(r.c0, a.c0, t0); f6mul(t1, a.c1, t0); f6neg(r.c1, t1);
}
// a <- a (c0 + (d0 + d1 v) w): 13 Fq2 products
ZK_PFN void f12mul034(fe12 &f, const fe2 &c0, const fe2 &d0, const fe2 &d1) {
    fe6 a, b, e;
    f2mul(a.c0, f.c0.c0, c0); f2mul(a.c1, f.c0.c1, c0); f2mul(a.c2, f.c0.c2, c0);
    f6mul01(b, f.c1, d0, d1);
    f6add(e, f.c0, f.c1);
    f6mul01(e, e, f2add(c0, d0), d1);
    f6sub(e, e, a); f6sub(f.c1, e, b);
    f6mulv(b, b); f6add(f.c0, a, b);
}
// a^(q^K): conjugate the coefficients for odd K, then a_ij *= xi^((2i + j)(q^K - 1)/6)
template <int K>
ZK_PFN void f12frob(fe12 &r, const fe12 &a) {
    fe2 t;
    r.c0.c0 = (K & 1) ? f2conj(a.c0.c0) : a.c0.c0;
    t = (K & 1) ? f2conj(a.c0.c1) : a.c0.c1; f2mul(r.c0.c1, t, frob_c<K, 2>());
    t = (K & 1) ? f2conj(a.c0.c2) : a.c0.c2; f2mul(r.c0.c2, t, frob_c<K, 4>());
    t = (K & 1) ? f2conj(a.c1.c0) : a.c1.c0; f2mul(r.c1.c0, t, frob_c<K, 1>());
    t = (K & 1) ? f2conj(a.c1.c1) : a.c1.c1; f2mul(r.c1.c1, t, frob_c<K, 3>());
    t = (K & 1) ? f2conj(a.c1.c2) : a.c1.c2; f2mul(r.c1.c2, t, frob_c<K, 5>());
}
// squaring in the cyclotomic subgroup (Granger-Scott): 9 Fq2 products (as three squarings in Fq4 = Fq2[y]/(y^2 - xi))
ZK_HD void fp4sqr(fe2 &t0, fe2 &t1, const fe2 &a, const fe2 &b) {
    fe2 ab, s;
    f2mul(ab, a, b);
    f2mul(s, f2add(a, b), f2add(f2mulxi(b), a));
    t0 = f2sub(f2sub(s, ab), f2mulxi(ab));             // a^2 + xi b^2
    t1 = f2dbl(ab);
}
ZK_PFN void f12cycsqr(fe12 &r, const fe12 &f) {
    fe2 t0, t1, t2, t3, t4, t5;
    fp4sqr(t0, t1, f.c0.c0, f.c1.c1);
    fp4sqr(t2, t3, f.c1.c0, f.c0.c2);
    fp4sqr(t4, t5, f.c0.c1, f.c1.c2);
    fe2 z;
    z = f2sub(t0, f.c0.c0); r.c0.c0 = f2add(f2dbl(z), t0);                       // 3 t0 - 2 z0
    z = f2add(t1, f.c1.c1); r.c1.c1 = f2add(f2dbl(z), t1);                       // 3 t1 + 2 z1
    const fe2 x5 = f2mulxi(t5);
    z = f2add(x5, f.c1.c0); const fe2 n10 = f2add(f2dbl(z), x5);                 // 3 xi t5 + 2 z2
    z = f2sub(t4, f.c0.c2); const fe2 n02 = f2add(f2dbl(z), t4);                 // 3 t4 - 2 z3
    z = f2sub(t2, f.c0.c1); const fe2 n01 = f2add(f2dbl(z), t2);                 // 3 t2 - 2 z4
    z = f2add(t3, f.c1.c2); const fe2 n12 = f2add(f2dbl(z), t3);                 // 3 t3 + 2 z5
    r.c1.c0 = n10; r.c0.c2 = n02; r.c0.c1 = n01; r.c1.c2 = n12;
}
ZK_PFN bool f12eq(const fe12 &a, const fe12 &b) {
    bool e = f2eq(a.c0.c0, b.c0.c0);
    e = f2eq(a.c0.c1, b.c0.c1) && e; e = f2eq(a.c0.c2, b.c0.c2) && e;
    e = f2eq(a.c1.c0, b.c1.c0) && e; e = f2eq(a.c1.c1, b.c1.c1) && e; e = f2eq(a.c1.c2, b.c1.c2) && e;
    return e;
}
ZK_PFN bool f12is_one(const fe12 &a) { const fe12 o = f12one(); return f12eq(a, o); }
ZK_PFN void f12canon(fe12 &a) {
    a.c0.c0 = Fq2::canon(a.c0.c0); a.c0.c1 = Fq2::canon(a.c0.c1); a.c0.c2 = Fq2::canon(a.c0.c2);
    a.c1.c0 = Fq2::canon(a.c1.c0); a.c1.c1 = Fq2::canon(a.c1.c1); a.c1.c2 = Fq2::canon(a.c1.c2);
}

// ---------------------------------------------------------------- final exponentiation
// conj(a^z) for a in the cyclotomic subgroup (there the conjugate is the inverse): a^(-z)
ZK_PFN void f12exp_negz(fe12 &r, const fe12 &a) {
    fe12 t = a;
    for (int i = 61; i >= 0; i--) {                    // z has 63 bits
        f12cycsqr(t, t);
        if ((BN_Z >> i) & 1) f12mul(t, t, a);
    }
    f12conj(r, t);
}
// f^((q^6 - 1)(q^2 + 1)): into the cyclotomic subgroup
ZK_PFN void final_exp_easy(fe12 &r, const fe12 &f) {
    fe12 t, c;
    f12inv(t, f); f12conj(c, f); f12mul(t, c, t);
    f12frob<2>(c, t); f12mul(r, c, t);
}
ZK_PFN void final_exp(fe12 &out, const fe12 &f) {
    fe12 r, y0, y1, y2, y3, y4, y5;
    final_exp_easy(r, f);
    f12exp_negz(y0, r);                                // r^-z
    f12cycsqr(y1, y0);                                 // r^-2z
    f12cycsqr(y2, y1);                                 // r^-4z
    f12mul(y3, y2, y1);                                // r^-6z
    f12exp_negz(y4, y3);                               // r^(6z^2)
    f12cycsqr(y5, y4);                                 // r^(12z^2)
    f12exp_negz(y2, y5);                               // r^(-12z^3)
    f12conj(y3, y3); f12conj(y2, y2);                  // r^(6z), r^(12z^3)
    f12mul(y2, y2, y4);                                // y7
    f12mul(y2, y2, y3);                                // y8
    f12mul(y0, y2, y1);                                // y9
    f12mul(y3, y2, y4);                                // y10
    f12mul(y3, y3, r);                                 // y11
    f12frob<1>(y5, y0); f12mul(y3, y5, y3);            // y13 = y9^q y11
    f12frob<2>(y5, y2); f12mul(y3, y5, y3);            // y14 = y8^(q^2) y13
    f12conj(r, r); f12mul(y0, r, y0);                  // y15 = r^-1 y9
    f12frob<3>(y5, y0); f12mul(out, y5, y3);
}

// ---------------------------------------------------------------- Miller loop
// T <- 2T; (a, b, c) = (-2YZ, 3X^2, 3b'Z^2 - Y^2)
ZK_PFN void dbl_step(G2Hom &r, LineC &l) {
    fe2 a, b, c, e, f, g, h, j, t;
    f2mul(a, r.x, r.y); f2muls(a, a, two_inv());
    f2sqr(b, r.y); f2sqr(c, r.z);
    f2mul(e, twist_b(), f2add(f2dbl(c), c));
    f = f2add(f2dbl(e), e);
    f2muls(g, f2add(b, f), two_inv());
    f2sqr(h, f2add(r.y, r.z)); h = f2sub(h, f2add(b, c));
    f2sqr(j, r.x);
    l.a = f2neg(h); l.b = f2add(f2dbl(j), j); l.c = f2sub(e, b);
    f2mul(r.x, a, f2sub(b, f));
    f2sqr(t, e); f2sqr(g, g); r.y = f2sub(g, f2add(f2dbl(t), t));
    f2mul(r.z, b, h);
}
// T <- T + Q; (a, b, c) = (lambda, -theta, theta x_Q - lambda y_Q), theta = Y - y_Q Z, lambda = X - x_Q Z
ZK_PFN void add_step(G2Hom &r, const G2::Affine &q, LineC &l) {
    fe2 th, la, c, d, e, f, g, h, t;
    f2mul(t, q.y, r.z); th = f2sub(r.y, t);
    f2mul(t, q.x, r.z); la = f2sub(r.x, t);
    f2sqr(c, th); f2sqr(d, la);
    f2mul(e, la, d); f2mul(f, r.z, c); f2mul(g, r.x, d);
    h = f2sub(f2add(e, f), f2dbl(g));
    f2mul(r.x, la, h);
    f2mul(t, th, f2sub(g, h)); f2mul(c, e, r.y); r.y = f2sub(t, c);
    f2mul(r.z, r.z, e);
    f2mul(t, th, q.x); f2mul(c, la, q.y);
    l.a = la; l.b = f2neg(th); l.c = f2sub(t, c);
}
// pi(Q) and -pi^2(Q) of the untwist-Frobenius-twist endomorphism
ZK_PFN void g2_frob1(G2::Affine &r, const G2::Affine &q) { f2mul(r.x, f2conj(q.x), frob_c<1, 2>()); f2mul(r.y, f2conj(q.y), frob_c<1, 3>()); }
ZK_PFN void g2_negfrob2(G2::Affine &r, const G2::Affine &q) { f2mul(r.x, q.x, frob_c<2, 2>()); r.y = q.y; }
// f <- f * line(P), or f unchanged when skip
ZK_PFN void ell(fe12 &f, const LineC &l, const G1::Affine &P, bool skip) {
    fe2 c0, d0;
    f2muls(c0, l.a, P.y); f2muls(d0, l.b, P.x);
    c0 = f2sel(skip, Fq2::one(), c0); d0 = f2sel(skip, Fq2::zero(), d0);
    const fe2 d1 = f2sel(skip, Fq2::zero(), l.c);
    f12mul034(f, c0, d0, d1);
}
ZK_HD bool pair_skip(const G1::Affine &P, const G2::Affine &Q) { return G1::is_inf(P) || G2::is_inf(Q); }

// step `idx` of the walk over Q (0 <= idx < MILLER_STEPS is implied by the caller's loop): the shared schedule of the
// variable-Q form, the fixed-Q form and the table writer.  KIND 0: doubling, 1: + Q, 2: + pi(Q), 3: - pi^2(Q)
ZK_PFN void walk_step(G2Hom &T, const G2::Affine &Q, int kind, LineC &l) {
    if (kind == 0) { dbl_step(T, l); return; }
    G2::Affine q = Q;
    if (kind == 2) g2_frob1(q, Q);
    if (kind == 3) g2_negfrob2(q, Q);
    add_step(T, q, l);
}
// the line coefficients of a fixed Q, MILLER_STEPS entries in loop order
ZK_PFN void miller_precompute(LineC *out, const G2::Affine &Q) {
    G2Hom T; T.x = Q.x; T.y = Q.y; T.z = Fq2::one();
    uint32_t idx = 0;
    for (int i = 63; i >= 0; i--) {
        walk_step(T, Q, 0, out[idx++]);
        if ((ATE_LOW >> i) & 1) walk_step(T, Q, 1, out[idx++]);
    }
    walk_step(T, Q, 2, out[idx++]);
    walk_step(T, Q, 3, out[idx++]);
}
// f = prod_{j < nv} ML(Pv[j], Qv[j]) * prod_{j < nf} ML(Pf[j], Q_j) with Q_j given by its table coef + j * MILLER_STEPS.
// T: nv entries of working storage.  nv, nf, fskip (bit j: fixed pair j is skipped whatever P is) are uniform.
ZK_PFN void miller_multi(fe12 &f, uint32_t nv, const G1::Affine *Pv, const G2::Affine *Qv, G2Hom *T,
                         uint32_t nf, const G1::Affine *Pf, const LineC *coef, uint32_t fskip) {
    f = f12one();
    for (uint32_t j = 0; j < nv; j++) { T[j].x = Qv[j].x; T[j].y = Qv[j].y; T[j].z = Fq2::one(); }
    uint32_t idx = 0;
    LineC l;
    for (int i = 63; i >= -2; i--) {
        const int nsub = i < 0 ? 1 : 1 + (int)((ATE_LOW >> i) & 1);
        for (int sub = 0; sub < nsub; sub++) {
            const int kind = i == -1 ? 2 : i == -2 ? 3 : sub;
            if (kind == 0 && i != 63) f12sqr(f, f);                              // (the first squaring would square 1)
            for (uint32_t j = 0; j < nv; j++) {
                walk_step(T[j], Qv[j], kind, l);
                ell(f, l, Pv[j], pair_skip(Pv[j], Qv[j]));
            }
            for (uint32_t j = 0; j < nf; j++) {
                l = coef[j * MILLER_STEPS + idx];
                ell(f, l, Pf[j], ((fskip >> j) & 1) || G1::is_inf(Pf[j]));
            }
            idx++;
        }
    }
}

// ---------------------------------------------------------------- [r]Q = O on the twist, by the walk above
// MSB-first double-and-add over r with the step functions of the Miller loop.  Their formulas are not complete; the walk
// stays exact because every exceptional case is itself a verdict: for Q of order r the partial multiples [m]Q, m < r, are
// neither O nor +-Q before the last addition, where T = -Q gives Z = 0.  If T = O or T = +-Q turns up earlier, Q has
// an order below r that is not 1, so [r]Q != O (r is prime).  Q = O itself is in the subgroup.
ZK_PFN bool g2_in_subgroup(const G2::Affine &Q) {
    G2Hom T; T.x = Q.x; T.y = Q.y; T.z = Fq2::one();
    LineC l;
    bool bad = false;
    for (int i = 252; i >= 0; i--) {                                             // r has 254 bits; bit 253 is T = Q
        bad = Fq2::lis_zero(T.z) || bad;
        dbl_step(T, l);
        if ((FrParams::p(i >> 5) >> (i & 31)) & 1) {
            bad = Fq2::lis_zero(T.z) || bad;
            add_step(T, Q, l);
            const bool lam0 = Fq2::lis_zero(l.a), th0 = Fq2::lis_zero(l.b);      // T = +-Q before the addition
            bad = (lam0 && (i != 0 || th0)) || bad;
        }
    }
    return G2::is_inf(Q) || (Fq2::lis_zero(T.z) && !bad);
}
ZK_HD bool g1_on_curve(const G1::Affine &p) {
    return G1::is_inf(p) || Fq::eq(Fq::canon(Fq::lsqr(p.y)), Fq::canon(Fq::ladd(Fq::lmul(Fq::lsqr(p.x), p.x), Fq::from_u64(3))));
}
ZK_PFN bool g2_on_curve(const G2::Affine &p) {
    fe2 yy, xx;
    f2sqr(yy, p.y); f2sqr(xx, p.x); f2mul(xx, xx, p.x);
    return G2::is_inf(p) || f2eq(yy, f2add(xx, twist_b()));
}

}  // namespace pairing
}  // namespace zk
