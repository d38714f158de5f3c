// verify_gpu.cpp -- batch Groth16 verification on the device: k proofs of ONE verification key in, k verdicts out.
//
// Equation per proof (the one of verify.cpp, e(alpha, beta) moved to the right-hand side and computed once per key):
//     FE( ML(A, B) ML(-acc, gamma) ML(-C, delta) ) == e(alpha, beta),   acc = gammaABC[0] + sum_j input_j gammaABC[j + 1]
// with the pairing of pairing.hpp: ML(A, B) walks B on the fly, gamma and delta come from line tables written at context creation.
//
// Two kernels per batch:
//   k_vfy_prepare  one quad per proof (blind.hpp's lane group): decodes the record (coordinates < q, inputs < r, to Montgomery), checks A
//                  and C against the curve, sums acc from the fixed-base window tables of gammaABC (blind_fixed<G1>; per-lane double-and-add
//                  for keys whose tables would pass the budget), one inversion to affine
//   k_vfy_pairing  one lane per proof: B on the twist and in the order-r subgroup ([r]B = O by pairing::g2_in_subgroup), the three-fold
//                  Miller loop, the final exponentiation, the comparison.  One lane per proof because the work is ~30 k Fq products with no
//                  parallelism worth a shuffle inside one Fq2 product and plenty across proofs: 16 384 proofs are one wave on every CU.
// A proof that fails a check gets verdict 0 by selection at the end; its lane runs the same instructions as its neighbours.
// Verdicts equal zk_verify's on the text zk_proof_to_json writes for the record, which is made of the coordinates alone: (0, 0) is the
// point at infinity and enters the product as the factor 1; the prover writes an infinite A, B or C as (0, 1) beside its *_inf flag, which
// is on neither curve, so such a record is rejected by the curve check like its text.
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <stdlib.h>
#include <string.h>
#include "bn254.hpp"
#define ZK_BLIND_NO_KERNELS                                     // the fixed-base tables and blind_fixed only
#include "blind.hpp"
#include "keygen.hpp"
#include "pairing.hpp"
#include "../../include/zkhip.h"

using namespace zk;
using namespace zk::pairing;

namespace {
constexpr uint32_t VFY_BLOCK = 64;
constexpr uint32_t VFY_MAX_BATCH = 1u << 20;
// the window tables of one gammaABC element take BLIND_ROWS x 64 bytes = 86 KiB; beyond this many bytes in all (about 3 000 inputs)
// the context keeps the points only and the prepare kernel multiplies by double-and-add.  ZK_VERIFY_TABLE_BUDGET=<bytes> overrides it.
constexpr size_t VFY_TABLE_BUDGET = (size_t)256 << 20;

int vfail(int code, const char *msg) { return fail_msg(code, msg); }

// what k_vfy_prepare hands to k_vfy_pairing (Montgomery, affine, (0, 0) = infinity)
struct alignas(16) VfyPoints {
    G1::Affine A, nAcc, nC;
    G2::Affine B;
    uint32_t ok, pad[3];
};

template <class P> ZK_HD bool lt_modulus(const fe &a) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.l[i] - P::p(i) - br; br = (t >> 32) & 1; }
    return br != 0;
}
ZK_HD fe load_words(const uint32_t *w) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = w[i];
    return r;
}
// coordinate c (0 .. 7: a_x, a_y, b_x_c0, b_x_c1, b_y_c0, b_y_c1, c_x, c_y) of a record: range check, Montgomery form
ZK_HD fe decode_coord(const zk_proof *pr, uint32_t c, bool &ok) {
    const fe v = load_words((const uint32_t *)pr + 8 * c);
    ok = lt_modulus<FqParams>(v) && ok;
    return Fq::to_mont(v);
}

struct PrepareArgs {
    const zk_proof *proofs; const fe *inputs; const uint8_t *flags;
    const G1::Affine *ic; const G1::Affine *tables;             // tables == nullptr: double-and-add from ic
    uint32_t nIn, k;
    VfyPoints *out;
};

__global__ void __launch_bounds__(VFY_BLOCK)
k_vfy_prepare(PrepareArgs a) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, p = tid / BLIND_Q, ql = tid & (BLIND_Q - 1);
    if (p >= a.k) return;                                        // (whole quads leave together)
    const zk_proof *pr = a.proofs + p;
    bool ok = a.flags[p] != 0;                                   // (the *_inf flags are not read: see the header of this file)
    VfyPoints v;
    v.A.x = decode_coord(pr, 0, ok); v.A.y = decode_coord(pr, 1, ok);
    v.B.x.c0 = decode_coord(pr, 2, ok); v.B.x.c1 = decode_coord(pr, 3, ok);
    v.B.y.c0 = decode_coord(pr, 4, ok); v.B.y.c1 = decode_coord(pr, 5, ok);
    G1::Affine Cc;
    Cc.x = decode_coord(pr, 6, ok); Cc.y = decode_coord(pr, 7, ok);
    ok = g1_on_curve(v.A) && ok;
    ok = g1_on_curve(Cc) && ok;
    G1::XYZZ acc = G1::from_affine(a.ic[0]);
    for (uint32_t j = 0; j < a.nIn; j++) {
        const fe s = a.inputs[(size_t)p * a.nIn + j];
        ok = lt_modulus<FrParams>(s) && ok;
        G1::XYZZ t;
        if (a.tables) t = blind_fixed<G1>(s, a.tables + (size_t)j * BLIND_ROWS, ql);
        else {
            const G1::Affine base = a.ic[j + 1];
            t = G1::infinity();
            for (uint32_t i = 256; i-- > 0;) {
                t = G1::dblQ<BLIND_Q>(t, ql);
                if (blind_bit(s, i)) t = G1::maddQ<BLIND_Q>(t, base, ql);
            }
        }
        acc = G1::addQ<BLIND_Q>(acc, t, ql);
    }
    v.nAcc = G1::neg(G1::to_affine(acc));
    v.nC = G1::neg(Cc);
    v.ok = ok ? 1u : 0u; v.pad[0] = v.pad[1] = v.pad[2] = 0;
    if (ql == 0) a.out[p] = v;
}

// coef: 2 x MILLER_STEPS lines of gamma, delta; fskip bit j: that key element is the point at infinity; eab = e(alpha, beta)
__global__ void __launch_bounds__(VFY_BLOCK)
k_vfy_pairing(const VfyPoints *__restrict__ pts, const LineC *__restrict__ coef, uint32_t fskip, const fe12 *__restrict__ eab,
              uint32_t k, uint8_t *__restrict__ accepted) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= k) return;
    const VfyPoints v = pts[p];
    bool ok = v.ok != 0;
    ok = g2_on_curve(v.B) && ok;
    ok = g2_in_subgroup(v.B) && ok;
    G1::Affine Pf[2]; Pf[0] = v.nAcc; Pf[1] = v.nC;
    G2Hom T;
    fe12 f, g;
    miller_multi(f, 1, &v.A, &v.B, &T, 2, Pf, coef, fskip);
    final_exp(g, f);
    const fe12 want = *eab;
    ok = f12eq(g, want) && ok;
    accepted[p] = ok ? 1 : 0;
}

// line tables of nq fixed points (one lane each)
__global__ void __launch_bounds__(VFY_BLOCK)
k_pair_precompute(const G2::Affine *__restrict__ Q, uint32_t nq, LineC *__restrict__ coef) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nq) return;
    const G2::Affine q = Q[j];
    miller_precompute(coef + (size_t)j * MILLER_STEPS, q);
}
// product i of k: values[i] = FE(prod_j ML(g1[i n + j], g2[i n + j])) (canonical) when values != nullptr; is_one[i] when is_one != nullptr
__global__ void __launch_bounds__(VFY_BLOCK)
k_pair_product(const G1::Affine *__restrict__ g1, const G2::Affine *__restrict__ g2, uint32_t n, uint32_t k, G2Hom *__restrict__ work,
               fe12 *__restrict__ values, uint8_t *__restrict__ is_one) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    fe12 f, g;
    miller_multi(f, n, g1 + (size_t)i * n, g2 + (size_t)i * n, work + (size_t)i * n, 0, nullptr, nullptr, 0);
    final_exp(g, f);
    f12canon(g);
    if (values) values[i] = g;
    if (is_one) is_one[i] = f12is_one(g) ? 1 : 0;
}

int vfy_use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return vfail(ZK_ERR_NODEVICE, "no HIP device (this library has no CPU path)");
    if (device < 0 || device >= n) return vfail(ZK_ERR_ARG, "device ordinal out of range");
    ZK_HIP(hipSetDevice(device));
    return ZK_OK;
}
bool host_g2_on_curve(const G2::Affine &p) { return g2_on_curve(p); }

template <class T> struct DevBuf {                              // frees on scope exit unless released
    T *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t count) { if (hipMalloc(&p, sizeof(T) * (count ? count : 1)) != hipSuccess) { p = nullptr; return vfail(ZK_ERR_NOMEM, "device allocation failed"); } return ZK_OK; }
    T *release() { T *r = p; p = nullptr; return r; }
};
}  // namespace

struct zk_vctx {
    int device = 0;
    uint32_t max_batch = 0, nIn = 0, fskip = 0;
    hipStream_t st = nullptr;
    G1::Affine *d_ic = nullptr, *d_tables = nullptr;
    LineC *d_coef = nullptr;
    fe12 *d_eab = nullptr;
    zk_proof *d_proofs = nullptr; fe *d_inputs = nullptr; uint8_t *d_flags = nullptr, *d_accepted = nullptr;
    VfyPoints *d_pts = nullptr;
    std::mutex mu;                                              // one batch at a time per context
    ~zk_vctx() {
        void *bufs[] = {d_ic, d_tables, d_coef, d_eab, d_proofs, d_inputs, d_flags, d_accepted, d_pts};
        for (void *b : bufs) if (b) (void)hipFree(b);
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {
int vctx_build(zk_vctx &v, const zk_vk &vk) {
    const size_t nIC = vk.gamma_abc.size();
    v.nIn = (uint32_t)(nIC - 1);
    ZK_HIP(hipStreamCreateWithFlags(&v.st, hipStreamNonBlocking));
    ZK_HIP(hipMalloc(&v.d_ic, sizeof(G1::Affine) * nIC));
    ZK_HIP(hipMemcpy(v.d_ic, vk.gamma_abc.data(), sizeof(G1::Affine) * nIC, hipMemcpyHostToDevice));
    size_t budget = VFY_TABLE_BUDGET;
    if (const char *e = getenv("ZK_VERIFY_TABLE_BUDGET")) budget = (size_t)strtoull(e, nullptr, 10);
    const size_t table_bytes = (size_t)v.nIn * BLIND_ROWS * sizeof(G1::Affine);
    if (v.nIn && table_bytes <= budget) {
        ZK_HIP(hipMalloc(&v.d_tables, table_bytes));
        std::vector<G1::Affine> T;
        for (uint32_t j = 0; j < v.nIn; j++) {
            blind_table_host<G1>(vk.gamma_abc[j + 1], T);
            ZK_HIP(hipMemcpy(v.d_tables + (size_t)j * BLIND_ROWS, T.data(), sizeof(G1::Affine) * BLIND_ROWS, hipMemcpyHostToDevice));
        }
    }
    // line tables of gamma and delta, e(alpha, beta): on the device, by the code every proof goes through
    const G2::Affine fixedQ[2] = {vk.gamma_g2, vk.delta_g2};
    v.fskip = (G2::is_inf(vk.gamma_g2) ? 1u : 0u) | (G2::is_inf(vk.delta_g2) ? 2u : 0u);
    DevBuf<G2::Affine> dq; DevBuf<G1::Affine> dp; DevBuf<G2Hom> dwork;
    ZK_TRY(dq.alloc(3)); ZK_TRY(dp.alloc(1)); ZK_TRY(dwork.alloc(1));
    ZK_HIP(hipMemcpy(dq.p, fixedQ, sizeof(fixedQ), hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(dq.p + 2, &vk.beta_g2, sizeof(G2::Affine), hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(dp.p, &vk.alpha_g1, sizeof(G1::Affine), hipMemcpyHostToDevice));
    ZK_HIP(hipMalloc(&v.d_coef, sizeof(LineC) * 2 * MILLER_STEPS));
    ZK_HIP(hipMalloc(&v.d_eab, sizeof(fe12)));
    ZK_LAUNCH(k_pair_precompute, 1, VFY_BLOCK, v.st, (const G2::Affine *)dq.p, 2u, v.d_coef);
    ZK_LAUNCH(k_pair_product, 1, VFY_BLOCK, v.st, (const G1::Affine *)dp.p, (const G2::Affine *)(dq.p + 2), 1u, 1u, dwork.p, v.d_eab, (uint8_t *)nullptr);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(v.st));
    // staging for max_batch proofs
    ZK_HIP(hipMalloc(&v.d_proofs, sizeof(zk_proof) * (size_t)v.max_batch));
    ZK_HIP(hipMalloc(&v.d_inputs, sizeof(fe) * ((size_t)v.max_batch * v.nIn + 1)));
    ZK_HIP(hipMalloc(&v.d_flags, v.max_batch));
    ZK_HIP(hipMalloc(&v.d_accepted, v.max_batch));
    ZK_HIP(hipMalloc(&v.d_pts, sizeof(VfyPoints) * (size_t)v.max_batch));
    return ZK_OK;
}

// uploads k records and runs k_vfy_prepare into d_pts (the caller holds the context's lock and has made its device current)
int vctx_prepare(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs, const uint8_t *flags, uint32_t k) {
    ZK_HIP(hipMemcpyAsync(v->d_proofs, proofs, sizeof(zk_proof) * (size_t)k, hipMemcpyHostToDevice, v->st));
    if (v->nIn) ZK_HIP(hipMemcpyAsync(v->d_inputs, inputs, sizeof(fe) * (size_t)k * v->nIn, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(v->d_flags, flags, k, hipMemcpyHostToDevice, v->st));
    PrepareArgs a;
    a.proofs = v->d_proofs; a.inputs = v->d_inputs; a.flags = v->d_flags; a.ic = v->d_ic; a.tables = v->d_tables;
    a.nIn = v->nIn; a.k = k; a.out = v->d_pts;
    ZK_LAUNCH(k_vfy_prepare, zk_div_up((uint64_t)k * BLIND_Q, VFY_BLOCK), VFY_BLOCK, v->st, a);
    return ZK_OK;
}

int vctx_run(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs, const uint8_t *flags, uint32_t k, uint8_t *accepted) {
    std::lock_guard<std::mutex> lk(v->mu);
    ZK_TRY(vfy_use_device(v->device));
    ZK_TRY(vctx_prepare(v, proofs, inputs, flags, k));
    ZK_LAUNCH(k_vfy_pairing, zk_div_up(k, VFY_BLOCK), VFY_BLOCK, v->st, (const VfyPoints *)v->d_pts, (const LineC *)v->d_coef, v->fskip,
              (const fe12 *)v->d_eab, k, v->d_accepted);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(accepted, v->d_accepted, k, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipStreamSynchronize(v->st));
    return ZK_OK;
}
}  // namespace

// ---- pairing probe (include/zkhip.h: TEST INFRASTRUCTURE).  One function of pairing.hpp per kernel instantiation, one lane per case, operands
// as given, raw result limbs back.  The kernels live in this unit so that they call the very ZK_PFN bodies k_vfy_pairing calls.
namespace {
constexpr uint32_t PP_MAX_CASES = 1u << 12;                     // (the fixed-Q ops keep 2 x MILLER_STEPS lines per lane in global memory)
ZK_HD fe2 pp_ld2(const fe *a) { fe2 r; r.c0 = a[0]; r.c1 = a[1]; return r; }
ZK_HD void pp_ld6(fe6 &r, const fe *a) { r.c0 = pp_ld2(a); r.c1 = pp_ld2(a + 2); r.c2 = pp_ld2(a + 4); }
ZK_HD void pp_ld12(fe12 &r, const fe *a) { pp_ld6(r.c0, a); pp_ld6(r.c1, a + 6); }
ZK_HD G1::Affine pp_ldg1(const fe *a) { G1::Affine p; p.x = a[0]; p.y = a[1]; return p; }
ZK_HD G2::Affine pp_ldg2(const fe *a) { G2::Affine p; p.x = pp_ld2(a); p.y = pp_ld2(a + 2); return p; }
ZK_HD void pp_st2(fe *o, const fe2 &v) { o[0] = v.c0; o[1] = v.c1; }
ZK_HD void pp_st6(fe *o, const fe6 &v) { pp_st2(o, v.c0); pp_st2(o + 2, v.c1); pp_st2(o + 4, v.c2); }
ZK_HD void pp_st12(fe *o, const fe12 &v) { pp_st6(o, v.c0); pp_st6(o + 6, v.c1); }
ZK_HD void pp_flag(fe *o, bool b) { fe r = Fq::zero(); r.l[0] = b ? 1u : 0u; o[0] = r; }
// a: the case's operand words, o: its result words (both in global memory), coef: the case's 2 x MILLER_STEPS lines (fixed-Q ops only)
#define ZK_PP_OP(NAME, NIN, NOUT, ...) \
    struct NAME { static constexpr uint32_t IN = NIN, OUT = NOUT; static ZK_HD void run(const fe *a, fe *o, LineC *coef) { __VA_ARGS__; } };
ZK_PP_OP(PpF6Mul, 12, 6, fe6 x, y, r; pp_ld6(x, a); pp_ld6(y, a + 6); f6mul(r, x, y); pp_st6(o, r))
ZK_PP_OP(PpF6MulAlias, 12, 6, fe6 x, y; pp_ld6(x, a); pp_ld6(y, a + 6); f6mul(x, x, y); pp_st6(o, x))
ZK_PP_OP(PpF6Mul01, 10, 6, fe6 x, r; pp_ld6(x, a); const fe2 b0 = pp_ld2(a + 6), b1 = pp_ld2(a + 8); f6mul01(r, x, b0, b1); pp_st6(o, r))
ZK_PP_OP(PpF6Inv, 6, 6, fe6 x, r; pp_ld6(x, a); f6inv(r, x); pp_st6(o, r))
ZK_PP_OP(PpF6MulV, 6, 6, fe6 x, r; pp_ld6(x, a); f6mulv(r, x); pp_st6(o, r))
ZK_PP_OP(PpF6Add, 12, 6, fe6 x, y, r; pp_ld6(x, a); pp_ld6(y, a + 6); f6add(r, x, y); pp_st6(o, r))
ZK_PP_OP(PpF6Sub, 12, 6, fe6 x, y, r; pp_ld6(x, a); pp_ld6(y, a + 6); f6sub(r, x, y); pp_st6(o, r))
ZK_PP_OP(PpF6Neg, 6, 6, fe6 x, r; pp_ld6(x, a); f6neg(r, x); pp_st6(o, r))
ZK_PP_OP(PpF2MulXi, 2, 2, pp_st2(o, f2mulxi(pp_ld2(a))))
ZK_PP_OP(PpF2MulS, 3, 2, fe2 r; const fe2 x = pp_ld2(a); const fe s = a[2]; f2muls(r, x, s); pp_st2(o, r))
ZK_PP_OP(PpF2Conj, 2, 2, pp_st2(o, f2conj(pp_ld2(a))))
ZK_PP_OP(PpF12Mul, 24, 12, fe12 x, y, r; pp_ld12(x, a); pp_ld12(y, a + 12); f12mul(r, x, y); pp_st12(o, r))
ZK_PP_OP(PpF12MulAlias, 24, 12, fe12 x, y; pp_ld12(x, a); pp_ld12(y, a + 12); f12mul(x, x, y); pp_st12(o, x))
ZK_PP_OP(PpF12Sqr, 12, 12, fe12 x, r; pp_ld12(x, a); f12sqr(r, x); pp_st12(o, r))
ZK_PP_OP(PpF12SqrAlias, 12, 12, fe12 x; pp_ld12(x, a); f12sqr(x, x); pp_st12(o, x))
ZK_PP_OP(PpF12Inv, 12, 12, fe12 x, r; pp_ld12(x, a); f12inv(r, x); pp_st12(o, r))
ZK_PP_OP(PpF12InvAlias, 12, 12, fe12 x; pp_ld12(x, a); f12inv(x, x); pp_st12(o, x))
ZK_PP_OP(PpF12Conj, 12, 12, fe12 x, r; pp_ld12(x, a); f12conj(r, x); pp_st12(o, r))
template <int K> ZK_PP_OP(PpF12Frob, 12, 12, fe12 x, r; pp_ld12(x, a); f12frob<K>(r, x); pp_st12(o, r))
ZK_PP_OP(PpF12CycSqr, 12, 12, fe12 x, r; pp_ld12(x, a); f12cycsqr(r, x); pp_st12(o, r))
ZK_PP_OP(PpF12CycSqrAlias, 12, 12, fe12 x; pp_ld12(x, a); f12cycsqr(x, x); pp_st12(o, x))
ZK_PP_OP(PpF12Mul034, 18, 12, fe12 x; pp_ld12(x, a); const fe2 c0 = pp_ld2(a + 12), d0 = pp_ld2(a + 14), d1 = pp_ld2(a + 16); f12mul034(x, c0, d0, d1); pp_st12(o, x))
ZK_PP_OP(PpF12Eq, 24, 1, fe12 x, y; pp_ld12(x, a); pp_ld12(y, a + 12); pp_flag(o, f12eq(x, y)))
ZK_PP_OP(PpF12IsOne, 12, 1, fe12 x; pp_ld12(x, a); pp_flag(o, f12is_one(x)))
ZK_PP_OP(PpF12Canon, 12, 12, fe12 x; pp_ld12(x, a); f12canon(x); pp_st12(o, x))
ZK_PP_OP(PpF12ExpNegZ, 12, 12, fe12 x, r; pp_ld12(x, a); f12exp_negz(r, x); pp_st12(o, r))
ZK_PP_OP(PpFinalExpEasy, 12, 12, fe12 x, r; pp_ld12(x, a); final_exp_easy(r, x); pp_st12(o, r))
ZK_PP_OP(PpFinalExp, 12, 12, fe12 x, r; pp_ld12(x, a); final_exp(r, x); pp_st12(o, r))
ZK_HD void pp_st_step(fe *o, const G2Hom &T, const LineC &l) {
    pp_st2(o, T.x); pp_st2(o + 2, T.y); pp_st2(o + 4, T.z); pp_st2(o + 6, l.a); pp_st2(o + 8, l.b); pp_st2(o + 10, l.c);
}
ZK_PP_OP(PpDblStep, 6, 12, G2Hom T; LineC l; T.x = pp_ld2(a); T.y = pp_ld2(a + 2); T.z = pp_ld2(a + 4); dbl_step(T, l); pp_st_step(o, T, l))
ZK_PP_OP(PpAddStep, 10, 12, G2Hom T; LineC l; T.x = pp_ld2(a); T.y = pp_ld2(a + 2); T.z = pp_ld2(a + 4); const G2::Affine q = pp_ldg2(a + 6);
         add_step(T, q, l); pp_st_step(o, T, l))
ZK_PP_OP(PpG2Frob1, 4, 4, G2::Affine r; const G2::Affine q = pp_ldg2(a); g2_frob1(r, q); pp_st2(o, r.x); pp_st2(o + 2, r.y))
ZK_PP_OP(PpG2NegFrob2, 4, 4, G2::Affine r; const G2::Affine q = pp_ldg2(a); g2_negfrob2(r, q); pp_st2(o, r.x); pp_st2(o + 2, r.y))
ZK_PP_OP(PpEll, 21, 12, fe12 f; pp_ld12(f, a); LineC l; l.a = pp_ld2(a + 12); l.b = pp_ld2(a + 14); l.c = pp_ld2(a + 16); const G1::Affine P = pp_ldg1(a + 18);
         ell(f, l, P, a[20].l[0] != 0); pp_st12(o, f))
// operands: NV points of G1, then NV points of G2 (the layout of zk_pairing_check's two arrays, per case)
template <uint32_t NV> ZK_PP_OP(PpMillerV, 6 * NV, 12, G1::Affine P[NV]; G2::Affine Q[NV]; G2Hom T[NV]; fe12 f;
         for (uint32_t j = 0; j < NV; j++) { P[j] = pp_ldg1(a + 2 * j); Q[j] = pp_ldg2(a + 2 * NV + 4 * j); }
         miller_multi(f, NV, P, Q, T, 0, nullptr, nullptr, 0); pp_st12(o, f))
// the fixed-Q route: the lane writes the line tables of its Q into coef, then walks them; the last operand word is fskip
template <uint32_t NF> ZK_PP_OP(PpMillerF, 6 * NF + 1, 12, G1::Affine P[NF]; fe12 f;
         for (uint32_t j = 0; j < NF; j++) { P[j] = pp_ldg1(a + 2 * j); const G2::Affine q = pp_ldg2(a + 2 * NF + 4 * j); miller_precompute(coef + j * MILLER_STEPS, q); }
         miller_multi(f, 0, nullptr, nullptr, nullptr, NF, P, coef, a[6 * NF].l[0]); pp_st12(o, f))
ZK_PP_OP(PpG2OnCurve, 4, 1, const G2::Affine q = pp_ldg2(a); pp_flag(o, g2_on_curve(q)))
ZK_PP_OP(PpG2InSubgroup, 4, 1, const G2::Affine q = pp_ldg2(a); pp_flag(o, g2_in_subgroup(q)))
ZK_PP_OP(PpG1OnCurve, 2, 1, pp_flag(o, g1_on_curve(pp_ldg1(a))))
#undef ZK_PP_OP

template <class Op>
__global__ void __launch_bounds__(VFY_BLOCK) k_pairing_probe(const fe *__restrict__ in, fe *__restrict__ out, uint32_t n, LineC *__restrict__ coef) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Op::run(in + (size_t)i * Op::IN, out + (size_t)i * Op::OUT, coef ? coef + (size_t)i * 2 * MILLER_STEPS : nullptr);
}
template <class Op> int pp_launch(const fe *d_in, uint32_t n, fe *d_out, LineC *d_coef) {
    ZK_LAUNCH((k_pairing_probe<Op>), zk_div_up(n, VFY_BLOCK), VFY_BLOCK, nullptr, d_in, d_out, n, d_coef);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// words per case in and out (in[i] = 0: no such op); ops 40 .. 42 are k_pair_product itself
constexpr uint32_t PP_OPS = 46, PP_FIXED0 = 38, PP_PRODUCT0 = 40;
const uint8_t pp_in[PP_OPS] = {12, 12, 10, 6, 6, 12, 12, 6, 2, 3, 2, 24, 24, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 18, 24, 12, 12, 12, 12, 12,
                               6, 10, 4, 4, 21, 6, 12, 18, 7, 13, 6, 12, 18, 4, 4, 2};
const uint8_t pp_out[PP_OPS] = {6, 6, 6, 6, 6, 6, 6, 6, 2, 2, 2, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 1, 1, 12, 12, 12, 12,
                                12, 12, 4, 4, 12, 12, 12, 12, 12, 12, 12, 12, 12, 1, 1, 1};
int pp_dispatch(int op, const fe *d_in, uint32_t n, fe *d_out, LineC *d_coef) {
    switch (op) {
    case 0: return pp_launch<PpF6Mul>(d_in, n, d_out, d_coef);
    case 1: return pp_launch<PpF6MulAlias>(d_in, n, d_out, d_coef);
    case 2: return pp_launch<PpF6Mul01>(d_in, n, d_out, d_coef);
    case 3: return pp_launch<PpF6Inv>(d_in, n, d_out, d_coef);
    case 4: return pp_launch<PpF6MulV>(d_in, n, d_out, d_coef);
    case 5: return pp_launch<PpF6Add>(d_in, n, d_out, d_coef);
    case 6: return pp_launch<PpF6Sub>(d_in, n, d_out, d_coef);
    case 7: return pp_launch<PpF6Neg>(d_in, n, d_out, d_coef);
    case 8: return pp_launch<PpF2MulXi>(d_in, n, d_out, d_coef);
    case 9: return pp_launch<PpF2MulS>(d_in, n, d_out, d_coef);
    case 10: return pp_launch<PpF2Conj>(d_in, n, d_out, d_coef);
    case 11: return pp_launch<PpF12Mul>(d_in, n, d_out, d_coef);
    case 12: return pp_launch<PpF12MulAlias>(d_in, n, d_out, d_coef);
    case 13: return pp_launch<PpF12Sqr>(d_in, n, d_out, d_coef);
    case 14: return pp_launch<PpF12SqrAlias>(d_in, n, d_out, d_coef);
    case 15: return pp_launch<PpF12Inv>(d_in, n, d_out, d_coef);
    case 16: return pp_launch<PpF12InvAlias>(d_in, n, d_out, d_coef);
    case 17: return pp_launch<PpF12Conj>(d_in, n, d_out, d_coef);
    case 18: return pp_launch<PpF12Frob<1>>(d_in, n, d_out, d_coef);
    case 19: return pp_launch<PpF12Frob<2>>(d_in, n, d_out, d_coef);
    case 20: return pp_launch<PpF12Frob<3>>(d_in, n, d_out, d_coef);
    case 21: return pp_launch<PpF12CycSqr>(d_in, n, d_out, d_coef);
    case 22: return pp_launch<PpF12CycSqrAlias>(d_in, n, d_out, d_coef);
    case 23: return pp_launch<PpF12Mul034>(d_in, n, d_out, d_coef);
    case 24: return pp_launch<PpF12Eq>(d_in, n, d_out, d_coef);
    case 25: return pp_launch<PpF12IsOne>(d_in, n, d_out, d_coef);
    case 26: return pp_launch<PpF12Canon>(d_in, n, d_out, d_coef);
    case 27: return pp_launch<PpF12ExpNegZ>(d_in, n, d_out, d_coef);
    case 28: return pp_launch<PpFinalExpEasy>(d_in, n, d_out, d_coef);
    case 29: return pp_launch<PpFinalExp>(d_in, n, d_out, d_coef);
    case 30: return pp_launch<PpDblStep>(d_in, n, d_out, d_coef);
    case 31: return pp_launch<PpAddStep>(d_in, n, d_out, d_coef);
    case 32: return pp_launch<PpG2Frob1>(d_in, n, d_out, d_coef);
    case 33: return pp_launch<PpG2NegFrob2>(d_in, n, d_out, d_coef);
    case 34: return pp_launch<PpEll>(d_in, n, d_out, d_coef);
    case 35: return pp_launch<PpMillerV<1>>(d_in, n, d_out, d_coef);
    case 36: return pp_launch<PpMillerV<2>>(d_in, n, d_out, d_coef);
    case 37: return pp_launch<PpMillerV<3>>(d_in, n, d_out, d_coef);
    case 38: return pp_launch<PpMillerF<1>>(d_in, n, d_out, d_coef);
    case 39: return pp_launch<PpMillerF<2>>(d_in, n, d_out, d_coef);
    case 43: return pp_launch<PpG2OnCurve>(d_in, n, d_out, d_coef);
    case 44: return pp_launch<PpG2InSubgroup>(d_in, n, d_out, d_coef);
    case 45: return pp_launch<PpG1OnCurve>(d_in, n, d_out, d_coef);
    }
    return vfail(ZK_ERR_ARG, "unknown pairing probe op");
}
// ops 40 .. 42: k_pair_product with `values` returned.  The case's operands are np G1 points then np G2 points: the kernel's two arrays
int pp_product(uint32_t np, const fe *in, uint32_t n, fe *out) {
    const size_t m = (size_t)n * np;
    std::vector<G1::Affine> g1(m);
    std::vector<G2::Affine> g2(m);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = 0; j < np; j++) {
            memcpy(&g1[(size_t)i * np + j], in + (size_t)i * 6 * np + 2 * j, sizeof(G1::Affine));
            memcpy(&g2[(size_t)i * np + j], in + (size_t)i * 6 * np + 2 * np + 4 * j, sizeof(G2::Affine));
        }
    DevBuf<G1::Affine> dp; DevBuf<G2::Affine> dq; DevBuf<G2Hom> dwork; DevBuf<fe12> dval;
    ZK_TRY(dp.alloc(m)); ZK_TRY(dq.alloc(m)); ZK_TRY(dwork.alloc(m)); ZK_TRY(dval.alloc(n));
    ZK_HIP(hipMemcpy(dp.p, g1.data(), sizeof(G1::Affine) * m, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(dq.p, g2.data(), sizeof(G2::Affine) * m, hipMemcpyHostToDevice));
    ZK_LAUNCH(k_pair_product, zk_div_up(n, VFY_BLOCK), VFY_BLOCK, nullptr, (const G1::Affine *)dp.p, (const G2::Affine *)dq.p, np, n, dwork.p, dval.p, (uint8_t *)nullptr);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, dval.p, sizeof(fe12) * (size_t)n, hipMemcpyDeviceToHost));
    return ZK_OK;
}
bool pp_shape(int op, uint32_t &in_words, uint32_t &out_words) {
    if (op < 0 || op >= (int)PP_OPS) return false;
    in_words = pp_in[op]; out_words = pp_out[op];
    return true;
}
}  // namespace

extern "C" int zk_vctx_create(const zk_vk *vk, int device, uint32_t max_batch, zk_vctx **out) try {
    if (!vk || !out) return vfail(ZK_ERR_ARG, "null argument");
    *out = nullptr;
    if (max_batch == 0 || max_batch > VFY_MAX_BATCH) return vfail(ZK_ERR_ARG, "max_batch must be in 1 .. 2^20");
    if (vk->gamma_abc.empty()) return vfail(ZK_ERR_FORMAT, "verification key without gammaABC");
    // the key's points lie on their curves (zk_verify checks the same and answers `not accepted`)
    bool ok = g1_on_curve(vk->alpha_g1) && host_g2_on_curve(vk->beta_g2) && host_g2_on_curve(vk->gamma_g2) && host_g2_on_curve(vk->delta_g2);
    for (const auto &p : vk->gamma_abc) ok = ok && g1_on_curve(p);
    if (!ok) return vfail(ZK_ERR_FORMAT, "verification key: a point is not on its curve");
    ZK_TRY(vfy_use_device(device));
    std::unique_ptr<zk_vctx> v(new zk_vctx());
    v->device = device; v->max_batch = max_batch;
    ZK_TRY(vctx_build(*v, *vk));
    *out = v.release();
    return ZK_OK;
} ZK_GUARD

extern "C" void zk_vctx_destroy(zk_vctx *v) try {
    if (!v) return;
    (void)vfy_use_device(v->device);
    delete v;
} ZK_GUARD_VOID

extern "C" int zk_verify_batch(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs_canon, uint32_t k, uint8_t *accepted) try {
    if (!v || !proofs || !accepted || (v->nIn && !inputs_canon)) return vfail(ZK_ERR_ARG, "null argument");
    if (k == 0 || k > v->max_batch) return vfail(ZK_ERR_ARG, "batch size must be in 1 .. max_batch");
    const std::vector<uint8_t> flags(k, 1);
    return vctx_run(v, proofs, inputs_canon, flags.data(), k, accepted);
} ZK_GUARD

extern "C" int zk_verify_batch_json(zk_vctx *v, const char *const *proof_json, uint32_t k, uint8_t *accepted) try {
    if (!v || !proof_json || !accepted) return vfail(ZK_ERR_ARG, "null argument");
    if (k == 0 || k > v->max_batch) return vfail(ZK_ERR_ARG, "batch size must be in 1 .. max_batch");
    for (uint32_t i = 0; i < k; i++) if (!proof_json[i]) return vfail(ZK_ERR_ARG, "null proof text");
    std::vector<zk_proof> proofs(k);
    std::vector<uint64_t> inputs(4 * (size_t)k * v->nIn + 4);
    std::vector<uint8_t> flags(k);
    for (uint32_t i = 0; i < k; i++) {
        uint32_t n = 0;
        const int rc = zk_proof_from_json(proof_json[i], &proofs[i], inputs.data() + 4 * (size_t)i * v->nIn, v->nIn, &n);
        flags[i] = rc == ZK_OK && n == v->nIn;                 // malformed text, a coordinate >= q, an input >= r, a wrong input count
        if (!flags[i]) { memset(&proofs[i], 0, sizeof(zk_proof)); memset(inputs.data() + 4 * (size_t)i * v->nIn, 0, 32 * (size_t)v->nIn); }
    }
    return vctx_run(v, proofs.data(), inputs.data(), flags.data(), k, accepted);
} ZK_GUARD

extern "C" int zk_pairing_check(const uint64_t *g1, const uint64_t *g2, uint32_t n, uint32_t k, int device, uint8_t *is_one) try {
    if (!g1 || !g2 || !is_one) return vfail(ZK_ERR_ARG, "null argument");
    if (n == 0 || k == 0 || (uint64_t)n * k > (1u << 24)) return vfail(ZK_ERR_ARG, "n and k must be positive, n k <= 2^24");
    ZK_TRY(vfy_use_device(device));
    const size_t m = (size_t)n * k;
    DevBuf<G1::Affine> dp; DevBuf<G2::Affine> dq; DevBuf<G2Hom> dwork; DevBuf<uint8_t> dout;
    ZK_TRY(dp.alloc(m)); ZK_TRY(dq.alloc(m)); ZK_TRY(dwork.alloc(m)); ZK_TRY(dout.alloc(k));
    ZK_HIP(hipMemcpy(dp.p, g1, sizeof(G1::Affine) * m, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(dq.p, g2, sizeof(G2::Affine) * m, hipMemcpyHostToDevice));
    ZK_LAUNCH(k_pair_product, zk_div_up(k, VFY_BLOCK), VFY_BLOCK, nullptr, (const G1::Affine *)dp.p, (const G2::Affine *)dq.p, n, k, dwork.p, (fe12 *)nullptr, dout.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(is_one, dout.p, k, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

// host-only: one operation of the Fq12 tower of pairing.hpp on canonical elements (12 x 4 u64, order c0.c0.c0, c0.c0.c1, c0.c1.c0, ...)
extern "C" int zk_pairing_tower_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) try {
    if (!a || !out || (op == 0 && !b)) return vfail(ZK_ERR_ARG, "null argument");
    auto load = [](const uint64_t *src) {
        fe12 r; fe *c = (fe *)&r;
        for (int i = 0; i < 12; i++) { fe t; memcpy(t.l, src + 4 * i, 32); c[i] = Fq::to_mont(t); }
        return r;
    };
    const fe12 x = load(a);
    fe12 r;
    switch (op) {
    case 0: { const fe12 y = load(b); f12mul(r, x, y); break; }
    case 1: f12sqr(r, x); break;
    case 2: f12inv(r, x); break;
    case 3: f12frob<1>(r, x); break;
    case 4: f12frob<2>(r, x); break;
    case 5: f12frob<3>(r, x); break;
    case 6: f12cycsqr(r, x); break;
    case 7: final_exp_easy(r, x); break;
    case 8: final_exp(r, x); break;
    case 9: f12conj(r, x); break;
    default: return vfail(ZK_ERR_ARG, "unknown tower operation");
    }
    f12canon(r);
    const fe *c = (const fe *)&r;
    for (int i = 0; i < 12; i++) { const fe t = Fq::from_mont(c[i]); memcpy(out + 4 * i, t.l, 32); }
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_pairing_probe_shape(int op, uint32_t *in_words, uint32_t *out_words) try {
    if (!in_words || !out_words) return vfail(ZK_ERR_ARG, "null argument");
    if (!pp_shape(op, *in_words, *out_words)) return vfail(ZK_ERR_ARG, "unknown pairing probe op");
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_pairing_probe(int op, const uint64_t *in, uint32_t n, uint64_t *out, int device) try {
    static_assert(sizeof(fe12) == 12 * sizeof(fe) && sizeof(LineC) == 6 * sizeof(fe) && sizeof(G2::Affine) == 4 * sizeof(fe), "the probe's word layouts");
    uint32_t wi = 0, wo = 0;
    if (!pp_shape(op, wi, wo)) return vfail(ZK_ERR_ARG, "unknown pairing probe op");
    if (n > PP_MAX_CASES) return vfail(ZK_ERR_ARG, "the pairing probe takes at most 2^12 cases per call");
    if (n && (!in || !out)) return vfail(ZK_ERR_ARG, "null argument");
    ZK_TRY(vfy_use_device(device));
    if (!n) return ZK_OK;
    if (op >= (int)PP_PRODUCT0 && op < (int)PP_PRODUCT0 + 3) return pp_product((uint32_t)op - PP_PRODUCT0 + 1, (const fe *)in, n, (fe *)out);
    DevBuf<fe> din, dout; DevBuf<LineC> dcoef;
    ZK_TRY(din.alloc((size_t)n * wi)); ZK_TRY(dout.alloc((size_t)n * wo));
    const bool fixed = op == (int)PP_FIXED0 || op == (int)PP_FIXED0 + 1;
    if (fixed) ZK_TRY(dcoef.alloc((size_t)n * 2 * MILLER_STEPS));
    ZK_HIP(hipMemcpy(din.p, in, sizeof(fe) * (size_t)n * wi, hipMemcpyHostToDevice));
    ZK_TRY(pp_dispatch(op, din.p, n, dout.p, fixed ? dcoef.p : nullptr));
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, dout.p, sizeof(fe) * (size_t)n * wo, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_vctx_probe_prepare(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs_canon, uint32_t k, uint64_t *out_points) try {
    static_assert(sizeof(VfyPoints) == 42 * sizeof(uint64_t), "the record zk_vctx_probe_prepare documents");
    if (!v || !proofs || !out_points || (v->nIn && !inputs_canon)) return vfail(ZK_ERR_ARG, "null argument");
    if (k == 0 || k > v->max_batch) return vfail(ZK_ERR_ARG, "batch size must be in 1 .. max_batch");
    const std::vector<uint8_t> flags(k, 1);
    std::lock_guard<std::mutex> lk(v->mu);
    ZK_TRY(vfy_use_device(v->device));
    ZK_TRY(vctx_prepare(v, proofs, inputs_canon, flags.data(), k));
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(out_points, v->d_pts, sizeof(VfyPoints) * (size_t)k, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipStreamSynchronize(v->st));
    return ZK_OK;
} ZK_GUARD
