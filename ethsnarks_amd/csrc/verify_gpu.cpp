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

int vctx_run(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs, const uint8_t *flags, uint32_t k, uint8_t *accepted) {
    std::lock_guard<std::mutex> lk(v->mu);
    ZK_TRY(vfy_use_device(v->device));
    ZK_HIP(hipMemcpyAsync(v->d_proofs, proofs, sizeof(zk_proof) * (size_t)k, hipMemcpyHostToDevice, v->st));
    if (v->nIn) ZK_HIP(hipMemcpyAsync(v->d_inputs, inputs, sizeof(fe) * (size_t)k * v->nIn, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(v->d_flags, flags, k, hipMemcpyHostToDevice, v->st));
    PrepareArgs a;
    a.proofs = v->d_proofs; a.inputs = v->d_inputs; a.flags = v->d_flags; a.ic = v->d_ic; a.tables = v->d_tables;
    a.nIn = v->nIn; a.k = k; a.out = v->d_pts;
    ZK_LAUNCH(k_vfy_prepare, zk_div_up((uint64_t)k * BLIND_Q, VFY_BLOCK), VFY_BLOCK, v->st, a);
    ZK_LAUNCH(k_vfy_pairing, zk_div_up(k, VFY_BLOCK), VFY_BLOCK, v->st, (const VfyPoints *)v->d_pts, (const LineC *)v->d_coef, v->fskip,
              (const fe12 *)v->d_eab, k, v->d_accepted);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(accepted, v->d_accepted, k, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipStreamSynchronize(v->st));
    return ZK_OK;
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
