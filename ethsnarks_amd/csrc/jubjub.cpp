// jubjub.cpp -- the host side of Baby JubJub behind zk_jj_*, zk_pedersen_* and zk_eddsa_* (include/zkhip.h).  Kernels: jubjub.hpp.
//
// Host-only work, done once per context with the strict field operations: hash-to-point (sha256, the from_y rule, a Tonelli-Shanks root, times the
// cofactor), the Pedersen tables (1 .. 4) 16^j B_s as affine points, the 16 multiples of the EdDSA base point, the MiMC constants of the seed
// "EdDSA_Verify.RAM", and -- on a handle's first zk_eddsa_sign_batch -- the signer's fixed-base table (0 .. 15) 16^j B (eddsa_sign.hpp), on a
// ZK_EDDSA_HASH handle's first zk_eddsa_fill_hash_witnesses the tables of its circuit (build_hash_fill_tables).  Per item the host only compares limbs with r; every field operation of a batch runs in ONE kernel launch.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>
#include <stdlib.h>
#include <string.h>
#include "bn254.hpp"
#include "jubjub.hpp"
#include "eddsa_sign.hpp"
#include "../../include/ethsnarks_hip/gadgets.hpp"              // the streaming sha256 and keccak256 (host code), as merkle.cpp uses them
#include "../../include/zkhip.h"

using namespace zk;
using namespace zk::jubjub;

static_assert(ZK_JJ_OP_ADD == OP_ADD && ZK_JJ_OP_DOUBLE == OP_DOUBLE && ZK_JJ_OP_NEGATE == OP_NEGATE, "zkhip.h and jubjub.hpp number the point operations alike");
static_assert(sizeof(zk_eddsa_layout) == sizeof(FillLayout) && sizeof(FillLayout) == 19 * sizeof(uint32_t), "zkhip.h and jubjub.hpp lay the witness row out alike");
static_assert(sizeof(zk_eddsa_pure_layout) == sizeof(PureLayout) && sizeof(PureLayout) == 26 * sizeof(uint32_t), "zkhip.h and jubjub.hpp lay the PureEdDSA witness row out alike");
static_assert(sizeof(zk_eddsa_hash_layout) == sizeof(HashLayout) && sizeof(HashLayout) == 32 * sizeof(uint32_t), "zkhip.h and jubjub.hpp lay the EdDSA (hash scheme) witness row out alike");
static_assert(ZK_EDDSA_MIMC == SCHEME_MIMC && ZK_EDDSA_PURE == SCHEME_PURE && ZK_EDDSA_HASH == SCHEME_HASH, "zkhip.h and jubjub.hpp number the schemes alike");

namespace {
constexpr uint32_t MAX_WINDOWS = SEG_WINDOWS * 256;             // 256 base points: a 6 MB table
constexpr uint32_t MAX_MSG_LEN = 4096;
constexpr uint32_t TWO_ADICITY = 28;                            // r - 1 = 2^28 q, q odd

int jfail(int code, const char *msg) { return fail_msg(code, msg); }

int jj_use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return jfail(ZK_ERR_NODEVICE, "no HIP device (this library has no CPU path)");
    if (device < 0 || device >= n) return jfail(ZK_ERR_ARG, "device ordinal out of range");
    ZK_HIP(hipSetDevice(device));
    return ZK_OK;
}

struct HP { fe x, y; };                                         // affine, Montgomery, canonical

fe limbs_to_fe(const uint64_t *v) { fe x; memcpy(x.l, v, 32); return x; }
bool all_below_modulus(const uint64_t *v, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) if (!merkle::fr_lt_modulus(limbs_to_fe(v + 4 * i))) return false;
    return true;
}
bool int_less(const fe &a, const fe &b) {
    for (int i = 7; i >= 0; i--) if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
}
// a 32-byte big-endian digest as a field element: value mod r, Montgomery
fe digest_to_mont(const uint8_t d[32]) {
    fe v;
    for (int i = 0; i < 8; i++) v.l[i] = ((uint32_t)d[28 - 4 * i] << 24) | ((uint32_t)d[29 - 4 * i] << 16) | ((uint32_t)d[30 - 4 * i] << 8) | d[31 - 4 * i];
    return Fr::to_mont(v);
}
void modulus_minus_one_shifted(uint32_t sh, uint32_t add, uint32_t e[8]) {   // ((r - 1) >> sh) + add, sh < 32
    uint32_t p[8];
    for (int i = 0; i < 8; i++) p[i] = FrParams::p(i);
    p[0] -= 1;
    for (int i = 0; i < 8; i++) e[i] = sh ? (p[i] >> sh) | (i < 7 ? p[i + 1] << (32 - sh) : 0u) : p[i];
    uint64_t c = add;
    for (int i = 0; i < 8 && c; i++) { c += e[i]; e[i] = (uint32_t)c; c >>= 32; }
}
// Tonelli-Shanks in Fr with the non-residue 5; false: a is not a square
bool fr_sqrt(const fe &a, fe &root) {
    if (Fr::is_zero(a)) { root = a; return true; }
    uint32_t e[8];
    modulus_minus_one_shifted(1, 0, e);
    if (!Fr::eq(Fr::pow(a, e), Fr::one())) return false;
    modulus_minus_one_shifted(TWO_ADICITY, 0, e);               // q
    fe c = Fr::pow(Fr::from_u64(5), e), t = Fr::pow(a, e);
    for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? e[i + 1] << 31 : 0u);
    uint64_t carry = 1;                                         // (q + 1) / 2 = (q >> 1) + 1, q odd
    for (int i = 0; i < 8 && carry; i++) { carry += e[i]; e[i] = (uint32_t)carry; carry >>= 32; }
    fe r = Fr::pow(a, e);
    uint32_t m = TWO_ADICITY;
    while (!Fr::eq(t, Fr::one())) {
        uint32_t i = 0;
        for (fe u = t; !Fr::eq(u, Fr::one()); u = Fr::sqr(u)) i++;
        fe b = c;
        for (uint32_t k = 0; k + i + 1 < m; k++) b = Fr::sqr(b);
        m = i; c = Fr::sqr(b); t = Fr::mul(t, c); r = Fr::mul(r, b);
    }
    root = r;
    return true;
}

void host_add(jpoint &a, jpoint b) { b.c[2] = Fr::mul(coef_d(), b.c[2]); jj_add(a, b.c, false); }
HP host_affine(const jpoint &p) {
    const fe zi = Fr::inv(p.c[3]);
    HP r; r.x = Fr::mul(p.c[0], zi); r.y = Fr::mul(p.c[1], zi);
    return r;
}
void put_point(const HP &p, uint64_t out[8]) {
    const fe x = Fr::from_mont(p.x), y = Fr::from_mont(p.y);
    memcpy(out, x.l, 32); memcpy(out + 4, y.l, 32);
}

// Point.from_hash: y = sha256(data) mod r, incremented until x^2 = (y^2 - 1) / (d y^2 - a) is a square; x the root with x > r - x; times 8
jpoint hash_to_point(const uint8_t *data, size_t len) {
    uint8_t dg[32];
    ethsnarks::hashes::sha256 h;
    h.update(data, len);
    h.digest(dg);
    fe y = digest_to_mont(dg), x;
    for (;; y = Fr::add(y, Fr::one())) {
        const fe ysq = Fr::sqr(y);
        const fe xsq = Fr::mul(Fr::sub(ysq, Fr::one()), Fr::inv(Fr::sub(Fr::mul(coef_d(), ysq), coef_a())));   // (d y^2 = a has no solution: a/d is no square)
        if (fr_sqrt(xsq, x)) break;
    }
    const fe nx = Fr::neg(x);
    if (int_less(Fr::from_mont(x), Fr::from_mont(nx))) x = nx;
    jpoint p;
    from_affine(p, x, y);
    for (int i = 0; i < 3; i++) jj_dbl(p, true);
    return p;
}
jpoint pedersen_basepoint(const std::string &name, uint32_t i) {
    char buf[40];
    snprintf(buf, sizeof(buf), "%-28s%04X", name.c_str(), i);
    return hash_to_point((const uint8_t *)buf, 32);
}
int check_name(const char *name) {
    if (!name) return jfail(ZK_ERR_ARG, "null argument");
    if (strlen(name) > 28) return jfail(ZK_ERR_ARG, "a Pedersen name has at most 28 bytes");
    return ZK_OK;
}

// projective points -> table entries (x, y, d x y), one inversion for all of them
void to_entries(const std::vector<jpoint> &pts, std::vector<fe> &out) {
    const size_t n = pts.size();
    std::vector<fe> pre(n);
    fe run = Fr::one();
    for (size_t i = 0; i < n; i++) { pre[i] = run; run = Fr::mul(run, pts[i].c[3]); }
    fe inv = Fr::inv(run);
    out.resize(3 * n);
    for (size_t i = n; i-- > 0;) {
        const fe zi = Fr::mul(inv, pre[i]);
        inv = Fr::mul(inv, pts[i].c[3]);
        const fe x = Fr::mul(pts[i].c[0], zi), y = Fr::mul(pts[i].c[1], zi);
        out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = Fr::mul(coef_d(), Fr::mul(x, y));
    }
}
// entries (j 4 + m) of the windows j = 0 .. windows - 1: (m + 1) 16^(j % 62) B_(j / 62)
void pedersen_table(const std::string &name, uint32_t windows, std::vector<fe> &out) {
    std::vector<jpoint> pts;
    pts.reserve((size_t)windows * 4);
    jpoint cur;
    for (uint32_t j = 0; j < windows; j++) {
        if (j % SEG_WINDOWS == 0) cur = pedersen_basepoint(name, j / SEG_WINDOWS);
        jpoint m2 = cur; jj_dbl(m2, true);
        jpoint m3 = m2; host_add(m3, cur);
        jpoint m4 = m2; jj_dbl(m4, true);
        pts.push_back(cur); pts.push_back(m2); pts.push_back(m3); pts.push_back(m4);
        cur = m4; jj_dbl(cur, true); jj_dbl(cur, true);
    }
    to_entries(pts, out);
}
// table entries (x, y, d x y) -> the Montgomery form (u, v) = ((1 + y) / (1 - y), u / x) of each point (EdwardsPoint::as_montgomery, scale 1), one
// inversion for all of them.  No table point has x = 0 or y = 1: each is a multiple below L of a point of prime order; false (and garbage in out)
// if one had
bool montgomery_entries(const std::vector<fe> &entries, std::vector<fe> &out) {
    const size_t n = entries.size() / 3;
    std::vector<fe> pre(n);
    fe run = Fr::one();
    for (size_t i = 0; i < n; i++) { pre[i] = run; run = Fr::mul(run, Fr::mul(Fr::sub(Fr::one(), entries[3 * i + 1]), entries[3 * i])); }
    const bool ok = !Fr::is_zero(run);
    fe inv = Fr::inv(run);
    out.resize(2 * n);
    for (size_t i = n; i-- > 0;) {
        const fe x = entries[3 * i], y = entries[3 * i + 1], omy = Fr::sub(Fr::one(), y);
        const fe di = Fr::mul(inv, pre[i]);                      // 1 / ((1 - y) x)
        inv = Fr::mul(inv, Fr::mul(omy, x));
        const fe u = Fr::mul(Fr::add(Fr::one(), y), Fr::mul(di, x));
        out[2 * i] = u; out[2 * i + 1] = Fr::mul(u, Fr::mul(di, omy));
    }
    return ok;
}
// window i of the circuit's fixed-base multiplication: identity, P, 2 P, 3 P with P = 4^i B, as table entries
void fixed_base_windows(const jpoint &B, std::vector<fe> &out) {
    std::vector<jpoint> w;
    w.reserve(4 * FB_WINDOWS);
    jpoint cur = B, zero;
    set_identity(zero);
    for (uint32_t i = 0; i < FB_WINDOWS; i++) {
        jpoint m2 = cur; jj_dbl(m2, true);
        jpoint m3 = m2; host_add(m3, cur);
        w.push_back(zero); w.push_back(cur); w.push_back(m2); w.push_back(m3);
        cur = m2; jj_dbl(cur, true);
    }
    to_entries(w, out);
}
// C_0 = keccak256(keccak256(seed)), C_{i+1} = keccak256(C_i) (mimc_constants of ethsnarks/mimc/permutation.py), Montgomery
void mimc_constants(const char *seed, fe *rc) {
    uint8_t dg[32], nx[32];
    ethsnarks::hashes::keccak256((const uint8_t *)seed, strlen(seed), dg);
    for (uint32_t i = 0; i < merkle::MIMC_ROUNDS; i++) {
        ethsnarks::hashes::keccak256(dg, 32, nx);
        memcpy(dg, nx, 32);
        rc[i] = digest_to_mont(dg);
    }
}

struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return ZK_OK;
        void *q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return jfail(ZK_ERR_NOMEM, "device allocation failed (Baby JubJub)"); }
        if (p) (void)hipFree(p);
        p = q; cap = bytes;
        return ZK_OK;
    }
    int upload(const void *src, size_t bytes) {
        ZK_TRY(ensure(bytes));
        ZK_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return ZK_OK;
    }
};
size_t align32(size_t v) { return (v + 31) & ~(size_t)31; }

bool point_on_curve(const uint64_t *p) {
    const fe x = Fr::to_mont(limbs_to_fe(p)), y = Fr::to_mont(limbs_to_fe(p + 4));
    return on_curve(x, y);
}
}  // namespace

struct zk_pedersen {
    int device = 0;
    uint32_t windows = 0;
    std::vector<fe> entries;                                    // the table as the device holds it
    DevBuf table, scratch;
    hipStream_t st = nullptr;
    ~zk_pedersen() { if (st) (void)hipStreamDestroy(st); }
};

struct zk_eddsa {
    int device = 0;
    uint32_t scheme = 0, msg_len = 0, ram_windows = 0, m_windows = 0;
    DevBuf consts, scratch;                                     // consts: btab | rc | ram table | m table | the 2-bit windows of B (MiMC, pure) | (u, v) of the ram table (pure)
    const fe *fbtab = nullptr;                                  // (0 .. 3) 4^i B, i = 0 .. 126: the tables of the circuit's fixed_base_mul
    const fe *mtab = nullptr;                                   // the Montgomery form of every ram table point: the lookups of the in-circuit Pedersen hash
    EddsaView view;
    jpoint base;                                                // B, for the signer's table
    DevBuf sign_tab;                                            // (0 .. 15) 16^j B, j = 0 .. 63 as (x, y, d x y): built by the first zk_eddsa_sign_batch
    DevBuf hash_fill_tab;                                       // (hash) fbtab | (u, v) of the ram table | (u, v) of the m table: built by the first zk_eddsa_fill_hash_witnesses
    const fe *m_mtab = nullptr;                                 // (hash) the Montgomery form of every m table point
    hipStream_t st = nullptr;
    ~zk_eddsa() { if (st) (void)hipStreamDestroy(st); }
};

extern "C" int zk_jj_hash_to_point(const uint8_t *data, size_t len, uint64_t out[8]) try {
    if ((len && !data) || !out) return jfail(ZK_ERR_ARG, "null argument");
    put_point(host_affine(hash_to_point(data, len)), out);
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_jj_pedersen_basepoint(const char *name, uint32_t i, uint64_t out[8]) try {
    ZK_TRY(check_name(name));
    if (!out) return jfail(ZK_ERR_ARG, "null argument");
    if (i > 0xFFFF) return jfail(ZK_ERR_ARG, "a Pedersen base point index is at most 0xFFFF");
    put_point(host_affine(pedersen_basepoint(name, i)), out);
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_jj_point_op(int op, const uint64_t *p, const uint64_t *q, uint32_t n, int device, uint64_t *out) try {
    if (op != OP_ADD && op != OP_DOUBLE && op != OP_NEGATE) return jfail(ZK_ERR_ARG, "unknown point operation");
    if (!p || !out || (op == OP_ADD && !q)) return jfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(p, 2 * (uint64_t)n) || (op == OP_ADD && !all_below_modulus(q, 2 * (uint64_t)n))) return jfail(ZK_ERR_ARG, "a coordinate is not below the Fr modulus");
    ZK_TRY(jj_use_device(device));
    const size_t bytes = 2 * sizeof(fe) * (size_t)n;
    DevBuf b;
    ZK_TRY(b.ensure(3 * bytes + 32));
    char *d = (char *)b.p;
    uint32_t *bad = (uint32_t *)(d + 3 * bytes);
    ZK_HIP(hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
    if (op == OP_ADD) ZK_HIP(hipMemcpy(d + bytes, q, bytes, hipMemcpyHostToDevice));
    ZK_HIP(hipMemset(bad, 0, 4));
    ZK_LAUNCH(k_jj_point_op, zk_div_up(n, BLOCK), BLOCK, nullptr, op, (const fe *)d, (const fe *)(d + bytes), n, (fe *)(d + 2 * bytes), bad);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    uint32_t nbad = 0;
    ZK_HIP(hipMemcpy(&nbad, bad, 4, hipMemcpyDeviceToHost));
    if (nbad) return jfail(ZK_ERR_ARG, "a point is not on the curve");
    ZK_HIP(hipMemcpy(out, d + 2 * bytes, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_jj_scalar_mul(const uint64_t *points, const uint64_t *scalars, uint32_t n, int device, uint64_t *out) try {
    if (!points || !scalars || !out) return jfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(points, 2 * (uint64_t)n)) return jfail(ZK_ERR_ARG, "a coordinate is not below the Fr modulus");
    ZK_TRY(jj_use_device(device));
    const size_t pb = 2 * sizeof(fe) * (size_t)n, sb = sizeof(fe) * (size_t)n;
    DevBuf b;
    ZK_TRY(b.ensure(2 * pb + sb + 32));
    char *d = (char *)b.p;
    uint32_t *bad = (uint32_t *)(d + 2 * pb + sb);
    ZK_HIP(hipMemcpy(d, points, pb, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d + pb, scalars, sb, hipMemcpyHostToDevice));
    ZK_HIP(hipMemset(bad, 0, 4));
    ZK_LAUNCH(k_jj_scalar_mul, zk_div_up(n, BLOCK), BLOCK, nullptr, (const fe *)d, (const fe *)(d + pb), n, (fe *)(d + pb + sb), bad);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    uint32_t nbad = 0;
    ZK_HIP(hipMemcpy(&nbad, bad, 4, hipMemcpyDeviceToHost));
    if (nbad) return jfail(ZK_ERR_ARG, "a point is not on the curve");
    ZK_HIP(hipMemcpy(out, d + pb + sb, pb, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_pedersen_create(const char *name, uint32_t max_windows, int device, zk_pedersen **out) try {
    if (!out) return jfail(ZK_ERR_ARG, "null argument");
    *out = nullptr;
    ZK_TRY(check_name(name));
    if (max_windows < 1 || max_windows > MAX_WINDOWS) return jfail(ZK_ERR_ARG, "max_windows must be in 1 .. 15872 (256 base points)");
    ZK_TRY(jj_use_device(device));
    std::unique_ptr<zk_pedersen> h(new zk_pedersen());
    h->device = device; h->windows = max_windows;
    pedersen_table(name, max_windows, h->entries);
    ZK_HIP(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
    ZK_TRY(h->table.upload(h->entries.data(), sizeof(fe) * h->entries.size()));
    *out = h.release();
    return ZK_OK;
} ZK_GUARD

extern "C" void zk_pedersen_free(zk_pedersen *h) try {
    if (!h) return;
    (void)jj_use_device(h->device);
    delete h;
} ZK_GUARD_VOID

extern "C" int zk_pedersen_table(const zk_pedersen *h, uint32_t first_window, uint32_t n_windows, uint64_t *out) try {
    if (!h || !out) return jfail(ZK_ERR_ARG, "null argument");
    if (first_window > h->windows || n_windows > h->windows - first_window) return jfail(ZK_ERR_ARG, "the hasher has no such windows");
    for (size_t i = 0; i < (size_t)n_windows * 4; i++) {
        HP p; p.x = h->entries[3 * ((size_t)first_window * 4 + i)]; p.y = h->entries[3 * ((size_t)first_window * 4 + i) + 1];
        put_point(p, out + 8 * i);
    }
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_pedersen_hash(zk_pedersen *h, const uint8_t *windows, const uint32_t *counts, uint32_t stride, uint32_t n, uint64_t *out) try {
    if (!h || !windows || !out) return jfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    if (stride == 0 || (!counts && stride > h->windows)) return jfail(ZK_ERR_ARG, "a hash takes 1 .. max_windows windows");
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = counts ? counts[i] : stride;
        if (c == 0 || c > stride || c > h->windows) return jfail(ZK_ERR_ARG, "a window count is 0, above the stride or above the capacity of the hasher");
        for (uint32_t j = 0; j < c; j++) if (windows[(size_t)i * stride + j] > 7) return jfail(ZK_ERR_ARG, "a window is not in 0 .. 7");
    }
    ZK_TRY(jj_use_device(h->device));
    const size_t wb = align32((size_t)n * stride), cb = align32(sizeof(uint32_t) * (size_t)n), ob = 2 * sizeof(fe) * (size_t)n;
    ZK_TRY(h->scratch.ensure(wb + cb + ob));
    char *d = (char *)h->scratch.p;
    ZK_HIP(hipMemcpyAsync(d, windows, (size_t)n * stride, hipMemcpyHostToDevice, h->st));
    if (counts) ZK_HIP(hipMemcpyAsync(d + wb, counts, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, h->st));
    ZK_LAUNCH(k_jj_pedersen, zk_div_up(n, BLOCK), BLOCK, h->st, (const fe *)h->table.p, (const uint8_t *)d, counts ? (const uint32_t *)(d + wb) : (const uint32_t *)nullptr, stride, n, (fe *)(d + wb + cb));
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(out, d + wb + cb, ob, hipMemcpyDeviceToHost, h->st));
    ZK_HIP(hipStreamSynchronize(h->st));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_eddsa_create(int scheme, const uint64_t *B, uint32_t msg_len, int device, zk_eddsa **out) try {
    if (!out) return jfail(ZK_ERR_ARG, "null argument");
    *out = nullptr;
    if (scheme != SCHEME_MIMC && scheme != SCHEME_PURE && scheme != SCHEME_HASH) return jfail(ZK_ERR_ARG, "unknown EdDSA scheme");
    if (msg_len < 1 || msg_len > MAX_MSG_LEN) return jfail(ZK_ERR_ARG, "msg_len must be in 1 .. 4096");
    // Point.generator() of jubjub.py: x = 1654064012...5038935, y = 2081904537...7972311
    static const uint64_t GENERATOR[8] = {0x79f2349047d5c157ull, 0xc88fee14d607cbe7ull, 0x6e35bc47bd9afe6cull, 0x2491aba8d3a191a7ull,
                                          0x348dd8f7f99152d7ull, 0xf9a9d4ed0cb0c1d1ull, 0x18dbddfd24c35583ull, 0x2e07297f8d3c3d78ull};
    if (!B) B = GENERATOR;
    if (!all_below_modulus(B, 2) || !point_on_curve(B)) return jfail(ZK_ERR_ARG, "the base point is not a point of the curve");
    ZK_TRY(jj_use_device(device));
    std::unique_ptr<zk_eddsa> v(new zk_eddsa());
    v->device = device; v->scheme = (uint32_t)scheme; v->msg_len = msg_len;
    // i B, i = 0 .. 15
    std::vector<jpoint> mult(TABLE);
    set_identity(mult[0]);
    from_affine(mult[1], Fr::to_mont(limbs_to_fe(B)), Fr::to_mont(limbs_to_fe(B + 4)));
    for (uint32_t i = 2; i < TABLE; i++) { mult[i] = mult[i - 1]; host_add(mult[i], mult[1]); }
    v->base = mult[1];
    std::vector<fe> btab, ram, mt, rc(merkle::MIMC_ROUNDS);
    to_entries(mult, btab);
    if (scheme == SCHEME_MIMC) mimc_constants("EdDSA_Verify.RAM", rc.data());
    else {
        v->ram_windows = scheme == SCHEME_HASH ? (3 * FIELD_BITS + 2) / 3 : (2 * FIELD_BITS + 8 * msg_len + 2) / 3;
        pedersen_table("EdDSA_Verify.RAM", v->ram_windows, ram);
        if (scheme == SCHEME_HASH) { v->m_windows = (8 * msg_len + 2) / 3; pedersen_table("EdDSA_Verify.M", v->m_windows, mt); }
    }
    std::vector<fe> all(btab), fb, mont;
    if (scheme != SCHEME_HASH) fixed_base_windows(mult[1], fb); // (a ZK_EDDSA_HASH handle builds its circuit's tables on its first fill: build_hash_fill_tables)
    if (scheme == SCHEME_PURE) (void)montgomery_entries(ram, mont);
    const size_t o_rc = all.size(); all.insert(all.end(), rc.begin(), rc.end());
    const size_t o_ram = all.size(); all.insert(all.end(), ram.begin(), ram.end());
    const size_t o_m = all.size(); all.insert(all.end(), mt.begin(), mt.end());
    const size_t o_fb = all.size(); all.insert(all.end(), fb.begin(), fb.end());
    const size_t o_mont = all.size(); all.insert(all.end(), mont.begin(), mont.end());
    ZK_HIP(hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking));
    ZK_TRY(v->consts.upload(all.data(), sizeof(fe) * all.size()));
    const fe *d = (const fe *)v->consts.p;
    v->view.btab = d; v->view.rc = d + o_rc; v->view.ram_tab = d + o_ram; v->view.m_tab = d + o_m;
    if (scheme != SCHEME_HASH) v->fbtab = d + o_fb;
    if (scheme == SCHEME_PURE) v->mtab = d + o_mont;
    v->view.scheme = v->scheme; v->view.msg_len = msg_len; v->view.ram_windows = v->ram_windows; v->view.m_windows = v->m_windows;
    *out = v.release();
    return ZK_OK;
} ZK_GUARD

extern "C" void zk_eddsa_free(zk_eddsa *v) try {
    if (!v) return;
    (void)jj_use_device(v->device);
    delete v;
} ZK_GUARD_VOID

extern "C" int zk_eddsa_verify_batch(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const void *msgs, uint32_t n, uint8_t *verdicts) try {
    if (!v || !A || !R || !s || !msgs || !verdicts) return jfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(A, 2 * (uint64_t)n) || !all_below_modulus(R, 2 * (uint64_t)n)) return jfail(ZK_ERR_ARG, "a coordinate is not below the Fr modulus");
    if (!all_below_modulus(s, n)) return jfail(ZK_ERR_ARG, "an s is not below the Fr modulus");
    const bool mimc = v->scheme == SCHEME_MIMC;
    if (mimc && !all_below_modulus((const uint64_t *)msgs, (uint64_t)n * v->msg_len)) return jfail(ZK_ERR_ARG, "a message element is not below the Fr modulus");
    ZK_TRY(jj_use_device(v->device));
    const size_t pb = 2 * sizeof(fe) * (size_t)n, sb = sizeof(fe) * (size_t)n;
    const size_t mb = (size_t)n * v->msg_len * (mimc ? sizeof(fe) : 1), mb_al = align32(mb);
    ZK_TRY(v->scratch.ensure(2 * pb + sb + mb_al + align32(n)));
    char *d = (char *)v->scratch.p;
    char *dA = d, *dR = d + pb, *dS = d + 2 * pb, *dM = dS + sb, *dV = dM + mb_al;
    ZK_HIP(hipMemcpyAsync(dA, A, pb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dR, R, pb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dS, s, sb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dM, msgs, mb, hipMemcpyHostToDevice, v->st));
    ZK_LAUNCH(k_eddsa_verify, zk_div_up(n, BLOCK), BLOCK, v->st, v->view, (const fe *)dA, (const fe *)dR, (const fe *)dS, (const void *)dM, n, (uint8_t *)dV);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(verdicts, dV, n, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipStreamSynchronize(v->st));
    return ZK_OK;
} ZK_GUARD

// ---- the witness fills
namespace {
struct Seg { uint64_t at, len; };
// every segment of a row inside variables 1 .. n_vars, n_vars + 1 <= row_elems, no two segments overlapping.  own: the segments that only this
// circuit has; the chain's segments are added here.  The three blocks of a step of the variable-base multiplication must lie, disjoint, within
// one stride of the lowest of them.  A segment without elements (no padding bits, no Edwards adder of the message hash) is not there: its
// offset is not looked at
bool row_fits(std::vector<Seg> segs, const ChainLayout &C, uint32_t n_vars, uint64_t row_elems) {
    if ((uint64_t)n_vars + 1 > row_elems) return false;
    const uint64_t step0 = std::min(C.doubler_var0, std::min(C.cond_var0, C.adder_var0));
    const Seg step[3] = {{C.doubler_var0, DBL_VARS}, {C.cond_var0, 2}, {C.adder_var0, ADD_VARS}};
    for (int i = 0; i < 3; i++) {
        if (step[i].at + step[i].len > step0 + C.step_stride) return false;
        for (int j = 0; j < i; j++) if (step[i].at < step[j].at + step[j].len && step[j].at < step[i].at + step[i].len) return false;
    }
    const Seg chain[] = {{C.ax_var, 2}, {C.rx_var, 2}, {C.s_bit0, FIELD_BITS}, {C.validator_var0, VALIDATOR_VARS}, {C.window_var0, 2 * FB_WINDOWS},
                         {C.fixed_adder_var0, ADD_VARS * (FB_WINDOWS - 1)}, {C.cond0_var, 2}, {step0, (uint64_t)N_STEPS * C.step_stride},
                         {C.last_adder_var0, ADD_VARS}};
    segs.insert(segs.end(), std::begin(chain), std::end(chain));
    std::sort(segs.begin(), segs.end(), [](const Seg &a, const Seg &b) { return a.at < b.at; });
    uint64_t end = 1;                                           // variable 0 is ONE
    for (const Seg &g : segs) {
        if (g.len == 0) continue;
        if (g.at < end) return false;
        end = g.at + g.len;
    }
    return end <= (uint64_t)n_vars + 1;
}
// the segments of one in-circuit Pedersen hash of W windows: its windows, Montgomery adders, converters and Edwards adders
void hash_segs(std::vector<Seg> &segs, uint64_t W, uint32_t window_var0, uint32_t mont_adder_var0, uint32_t converter_var0, uint32_t edwards_adder_var0) {
    const uint64_t S = (W + SEG_WINDOWS - 1) / SEG_WINDOWS;
    segs.insert(segs.end(), {{window_var0, 2 * W}, {mont_adder_var0, MADD_VARS * (W - S)}, {converter_var0, 2 * S}, {edwards_adder_var0, ADD_VARS * (S - 1)}});
}
// the MiMC-EdDSA row
bool layout_fits(const FillLayout &L, uint32_t msg_len, uint64_t row_elems) {
    if (L.msg_len != msg_len) return false;
    uint32_t range_vars = 0;
    for (uint32_t i = 1; i + 1 < FIELD_BITS; i++) range_vars += modulus_m1_bit(i);
    if (range_vars != T_RANGE_VARS) return false;
    return row_fits({{L.msg_var0, msg_len}, {L.iv_var, 1}, {L.mimc_var0, (uint64_t)(4 + msg_len) * (1 + MIMC_ROUND_VARS)}, {L.t_bit0, T_BITS_VARS},
                     {L.t_range_var0, T_RANGE_VARS}}, chain_layout(L), L.n_vars, row_elems);
}
// the PureEdDSA row: the hash's segments sized by the window count of the verifier's msg_len
bool pure_layout_fits(const PureLayout &L, uint32_t msg_len, uint64_t row_elems) {
    if (L.msg_len != msg_len) return false;
    const uint64_t W = pure_windows(msg_len);
    std::vector<Seg> segs = {{L.msg_bit0, 8 * (uint64_t)msg_len}, {L.pad_bit0, 3 * W - 2 * FIELD_BITS - 8 * (uint64_t)msg_len}, {L.rx_bit0, T_BITS_VARS},
                             {L.rx_range_var0, T_RANGE_VARS}, {L.ax_bit0, T_BITS_VARS}, {L.ax_range_var0, T_RANGE_VARS}, {L.t_bit0, T_BITS_VARS},
                             {L.t_range_var0, T_RANGE_VARS}};
    hash_segs(segs, W, L.hash_window_var0, L.mont_adder_var0, L.converter_var0, L.edwards_adder_var0);
    return row_fits(segs, chain_layout(L), L.n_vars, row_elems);
}
// the EdDSA (hash scheme) row: the RAM hash over 3 x 254 bits and the message hash sized by the verifier's msg_len
bool hash_layout_fits(const HashLayout &L, uint32_t msg_len, uint64_t row_elems) {
    if (L.msg_len != msg_len) return false;
    const uint64_t Wm = hash_msg_windows(msg_len);
    std::vector<Seg> segs = {{L.msg_bit0, 8 * (uint64_t)msg_len}, {L.m_pad_bit0, 3 * Wm - 8 * (uint64_t)msg_len}, {L.m_bit0, T_BITS_VARS},
                             {L.m_range_var0, T_RANGE_VARS}, {L.rx_bit0, T_BITS_VARS}, {L.rx_range_var0, T_RANGE_VARS}, {L.ax_bit0, T_BITS_VARS},
                             {L.ax_range_var0, T_RANGE_VARS}, {L.t_bit0, T_BITS_VARS}, {L.t_range_var0, T_RANGE_VARS}};
    hash_segs(segs, Wm, L.m_window_var0, L.m_mont_adder_var0, L.m_converter_var0, L.m_edwards_adder_var0);
    hash_segs(segs, HASH_RAM_WINDOWS, L.hash_window_var0, L.mont_adder_var0, L.converter_var0, L.edwards_adder_var0);
    return row_fits(segs, chain_layout(L), L.n_vars, row_elems);
}

// a batch on the device: what a fill kernel reads and where its verdicts go
struct Staged { const fe *A, *R, *s; const void *msgs; uint8_t *verdicts; };
// what every fill does once its arguments are checked: A, R, s and the messages (msg_stride bytes an item) go to the handle's scratch, `launch`
// starts the kernel over them, the verdicts come back
template <class Launch>
int stage_and_fill(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const void *msgs, size_t msg_stride, uint32_t n, uint8_t *verdicts,
                   Launch launch) {
    const size_t pb = 2 * sizeof(fe) * (size_t)n, sb = sizeof(fe) * (size_t)n, mb = (size_t)n * msg_stride, mb_al = align32(mb);
    ZK_TRY(v->scratch.ensure(2 * pb + sb + mb_al + align32(n)));
    char *d = (char *)v->scratch.p;
    char *dA = d, *dR = d + pb, *dS = d + 2 * pb, *dM = dS + sb, *dV = dM + mb_al;
    ZK_HIP(hipMemcpyAsync(dA, A, pb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dR, R, pb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dS, s, sb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dM, msgs, mb, hipMemcpyHostToDevice, v->st));
    launch(Staged{(const fe *)dA, (const fe *)dR, (const fe *)dS, (const void *)dM, (uint8_t *)dV});
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(verdicts, dV, n, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipStreamSynchronize(v->st));
    return ZK_OK;
}

// zk_eddsa_fill_witnesses and zk_eddsa_fill_witnesses_wide behind the check of `lanes`: 1 launches k_eddsa_fill, 2 and 4 k_eddsa_fill_wide over
// workgroups of 64 x lanes threads
int fill_mimc(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const uint64_t *msgs, uint32_t n, void *d_w, uint64_t row_elems,
              const zk_eddsa_layout *layout, uint8_t *verdicts, uint32_t lanes) {
    if (!v || !A || !R || !s || !msgs || !d_w || !layout || !verdicts) return jfail(ZK_ERR_ARG, "null argument");
    if (v->scheme != SCHEME_MIMC) return jfail(ZK_ERR_ARG, "only a ZK_EDDSA_MIMC verifier has a circuit to fill witnesses of");
    FillLayout L;
    memcpy(&L, layout, sizeof(L));
    if (!layout_fits(L, v->msg_len, row_elems)) return jfail(ZK_ERR_ARG, "the layout does not fit the verifier's msg_len, overlaps itself or leaves the row");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(A, 2 * (uint64_t)n) || !all_below_modulus(R, 2 * (uint64_t)n)) return jfail(ZK_ERR_ARG, "a coordinate is not below the Fr modulus");
    if (!all_below_modulus(msgs, (uint64_t)n * v->msg_len)) return jfail(ZK_ERR_ARG, "a message element is not below the Fr modulus");
    ZK_TRY(jj_use_device(v->device));
    return stage_and_fill(v, A, R, s, msgs, sizeof(fe) * v->msg_len, n, verdicts, [&](const Staged &d) {
        if (lanes == 1) ZK_LAUNCH(k_eddsa_fill, zk_div_up(n, BLOCK), BLOCK, v->st, v->view, v->fbtab, L, d.A, d.R, d.s, (const fe *)d.msgs, n, (fe *)d_w, row_elems, d.verdicts);
        else if (lanes == 2) ZK_LAUNCH_SYNC((k_eddsa_fill_wide<2>), zk_div_up(n, BLOCK), BLOCK * 2, v->st, v->view, v->fbtab, L, d.A, d.R, d.s, (const fe *)d.msgs, n,
                                            (fe *)d_w, row_elems, d.verdicts);
        else ZK_LAUNCH_SYNC((k_eddsa_fill_wide<4>), zk_div_up(n, BLOCK), BLOCK * 4, v->st, v->view, v->fbtab, L, d.A, d.R, d.s, (const fe *)d.msgs, n, (fe *)d_w,
                            row_elems, d.verdicts);
    });
}

// what the fill of a ZK_EDDSA_HASH handle reads beyond the verifier's tables: the circuit's fixed-base windows and the Montgomery form of the two
// Pedersen tables (read back from the device: the handle keeps no host copy).  Built once, freed with the handle
int build_hash_fill_tables(zk_eddsa *v) {
    if (v->hash_fill_tab.p) return ZK_OK;
    const size_t n_ram = (size_t)v->ram_windows * 4 * 3, n_m = (size_t)v->m_windows * 4 * 3;
    std::vector<fe> ram(n_ram), mt(n_m), all, mont_ram, mont_m;
    ZK_HIP(hipMemcpy(ram.data(), v->view.ram_tab, sizeof(fe) * n_ram, hipMemcpyDeviceToHost));
    ZK_HIP(hipMemcpy(mt.data(), v->view.m_tab, sizeof(fe) * n_m, hipMemcpyDeviceToHost));
    fixed_base_windows(v->base, all);
    if (!montgomery_entries(ram, mont_ram) || !montgomery_entries(mt, mont_m))
        return jfail(ZK_ERR_INTERNAL, "a Pedersen table point has x = 0 or y = 1: it has no Montgomery form");
    const size_t o_ram = all.size(); all.insert(all.end(), mont_ram.begin(), mont_ram.end());
    const size_t o_m = all.size(); all.insert(all.end(), mont_m.begin(), mont_m.end());
    DevBuf b;
    ZK_TRY(b.upload(all.data(), sizeof(fe) * all.size()));
    std::swap(v->hash_fill_tab.p, b.p); std::swap(v->hash_fill_tab.cap, b.cap);
    const fe *d = (const fe *)v->hash_fill_tab.p;
    v->fbtab = d; v->mtab = d + o_ram; v->m_mtab = d + o_m;
    return ZK_OK;
}
}  // namespace

extern "C" int zk_eddsa_fill_witnesses(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const uint64_t *msgs, uint32_t n, void *d_w,
                                       uint64_t row_elems, const zk_eddsa_layout *layout, uint8_t *verdicts) try {
    return fill_mimc(v, A, R, s, msgs, n, d_w, row_elems, layout, verdicts, 1);
} ZK_GUARD

// zk_eddsa_fill_witnesses with `lanes` lanes per witness.  lanes is checked first, then that call's checks in its order; the same rows byte for byte
extern "C" int zk_eddsa_fill_witnesses_wide(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const uint64_t *msgs, uint32_t n, void *d_w,
                                            uint64_t row_elems, const zk_eddsa_layout *layout, uint8_t *verdicts, uint32_t lanes) try {
    if (lanes != 1 && lanes != 2 && lanes != 4) return jfail(ZK_ERR_ARG, "lanes per witness: 1, 2 or 4");
    return fill_mimc(v, A, R, s, msgs, n, d_w, row_elems, layout, verdicts, lanes);
} ZK_GUARD

extern "C" int zk_eddsa_fill_pure_witnesses(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const uint8_t *msgs, uint32_t n, void *d_w,
                                            uint64_t row_elems, const zk_eddsa_pure_layout *layout, uint8_t *verdicts) try {
    if (!v || !A || !R || !s || !msgs || !d_w || !layout || !verdicts) return jfail(ZK_ERR_ARG, "null argument");
    if (v->scheme != SCHEME_PURE) return jfail(ZK_ERR_ARG, "only a ZK_EDDSA_PURE verifier has a PureEdDSA circuit to fill witnesses of");
    PureLayout L;
    memcpy(&L, layout, sizeof(L));
    if (!pure_layout_fits(L, v->msg_len, row_elems)) return jfail(ZK_ERR_ARG, "the layout does not fit the verifier's msg_len, overlaps itself or leaves the row");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(A, 2 * (uint64_t)n) || !all_below_modulus(R, 2 * (uint64_t)n)) return jfail(ZK_ERR_ARG, "a coordinate is not below the Fr modulus");
    ZK_TRY(jj_use_device(v->device));
    return stage_and_fill(v, A, R, s, msgs, v->msg_len, n, verdicts, [&](const Staged &d) {
        ZK_LAUNCH(k_eddsa_fill_pure, zk_div_up(n, BLOCK), BLOCK, v->st, v->view, v->fbtab, v->mtab, L, d.A, d.R, d.s, (const uint8_t *)d.msgs, n, (fe *)d_w, row_elems,
                  d.verdicts);
    });
} ZK_GUARD

extern "C" int zk_eddsa_fill_hash_witnesses(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const uint8_t *msgs, uint32_t n, void *d_w,
                                            uint64_t row_elems, const zk_eddsa_hash_layout *layout, uint8_t *verdicts) try {
    if (!v || !layout) return jfail(ZK_ERR_ARG, "null argument");
    if (v->scheme != SCHEME_HASH) return jfail(ZK_ERR_ARG, "only a ZK_EDDSA_HASH verifier has an EdDSA circuit with the message hash in it to fill witnesses of");
    HashLayout L;
    memcpy(&L, layout, sizeof(L));
    if (!hash_layout_fits(L, v->msg_len, row_elems)) return jfail(ZK_ERR_ARG, "the layout does not fit the verifier's msg_len, overlaps itself or leaves the row");
    if (n == 0) return ZK_OK;
    if (!A || !R || !s || !msgs || !d_w || !verdicts) return jfail(ZK_ERR_ARG, "null argument");
    if (!all_below_modulus(A, 2 * (uint64_t)n) || !all_below_modulus(R, 2 * (uint64_t)n)) return jfail(ZK_ERR_ARG, "a coordinate is not below the Fr modulus");
    ZK_TRY(jj_use_device(v->device));
    ZK_TRY(build_hash_fill_tables(v));
    return stage_and_fill(v, A, R, s, msgs, v->msg_len, n, verdicts, [&](const Staged &d) {
        ZK_LAUNCH(k_eddsa_fill_hash, zk_div_up(n, BLOCK), BLOCK, v->st, v->view, v->fbtab, v->mtab, v->m_mtab, L, d.A, d.R, d.s, (const uint8_t *)d.msgs, n, (fe *)d_w,
                  row_elems, d.verdicts);
    });
} ZK_GUARD

// ---- the signer (eddsa_sign.hpp)
namespace {
bool key_in_range(const uint64_t *k) {                          // 0 < k < L
    static const uint64_t ORDER[4] = {0x677297dc392126f1ull, 0xab3eedb83920ee0aull, 0x370a08b6d0302b0bull, 0x060c89ce5c263405ull};
    if (!(k[0] | k[1] | k[2] | k[3])) return false;
    for (int i = 3; i >= 0; i--) if (k[i] != ORDER[i]) return k[i] < ORDER[i];
    return false;
}
// entry (j 16 + m) = m 16^j B, with the strict field operations like the Pedersen tables
int build_sign_table(zk_eddsa *v) {
    if (v->sign_tab.p) return ZK_OK;
    std::vector<jpoint> pts;
    pts.reserve(SIGN_TABLE_ENTRIES);
    jpoint cur = v->base, zero;
    set_identity(zero);
    for (uint32_t j = 0; j < N_WIN; j++) {
        pts.push_back(zero);
        pts.push_back(cur);
        for (uint32_t m = 2; m < TABLE; m++) { jpoint nx = pts.back(); host_add(nx, cur); pts.push_back(nx); }
        for (uint32_t b = 0; b < WIN; b++) jj_dbl(cur, true);
    }
    std::vector<fe> entries;
    to_entries(pts, entries);
    return v->sign_tab.upload(entries.data(), sizeof(fe) * entries.size());
}
// the device copies of the keys and of the nonces do not outlive the call, whichever way the call ends
struct WipeOnExit {
    void *p; size_t bytes; hipStream_t st;
    ~WipeOnExit() { if (p && bytes) { (void)hipMemsetAsync(p, 0, bytes, st); (void)hipStreamSynchronize(st); } }
};
}  // namespace

extern "C" int zk_eddsa_sign_batch(zk_eddsa *v, const uint64_t *keys, const void *msgs, uint32_t n, uint64_t *A, uint64_t *R, uint64_t *s) try {
    if (!v || !keys || !msgs || !A || !R || !s) return jfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    for (uint32_t i = 0; i < n; i++) if (!key_in_range(keys + 4 * (size_t)i)) return jfail(ZK_ERR_ARG, "a key is not in 1 .. L - 1");
    const bool mimc = v->scheme == SCHEME_MIMC;
    if (mimc && !all_below_modulus((const uint64_t *)msgs, (uint64_t)n * v->msg_len)) return jfail(ZK_ERR_ARG, "a message element is not below the Fr modulus");
    ZK_TRY(jj_use_device(v->device));
    ZK_TRY(build_sign_table(v));
    const size_t pb = 2 * sizeof(fe) * (size_t)n, sb = sizeof(fe) * (size_t)n;
    const size_t mb = (size_t)n * v->msg_len * (mimc ? sizeof(fe) : 1), mb_al = align32(mb);
    ZK_TRY(v->scratch.ensure(2 * sb + mb_al + 2 * pb + sb + (v->scheme == SCHEME_HASH ? pb : 0)));
    char *d = (char *)v->scratch.p;
    char *dK = d, *dN = dK + sb, *dM = dN + sb, *dA = dM + mb_al, *dR = dA + pb, *dS = dR + pb, *dP = dS + sb;
    WipeOnExit wipe{dK, 2 * sb, v->st};                         // keys | nonces: the kernel reads both from here at every use (eddsa_sign.hpp)
    ZK_HIP(hipMemcpyAsync(dK, keys, sb, hipMemcpyHostToDevice, v->st));
    ZK_HIP(hipMemcpyAsync(dM, msgs, mb, hipMemcpyHostToDevice, v->st));
    ZK_LAUNCH(k_eddsa_sign, zk_div_up(n, BLOCK), BLOCK, v->st, v->view, (const fe *)v->sign_tab.p, (const fe *)dK, (fe *)dN, (const void *)dM, n, (fe *)dA, (fe *)dR, (fe *)dS,
              v->scheme == SCHEME_HASH ? (fe *)dP : (fe *)nullptr);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(v->st));
    ZK_HIP(hipMemcpyAsync(A, dA, pb, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipMemcpyAsync(R, dR, pb, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipMemcpyAsync(s, dS, sb, hipMemcpyDeviceToHost, v->st));
    ZK_HIP(hipStreamSynchronize(v->st));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_eddsa_sign_probe(int op, const void *a, const void *b, const void *c, uint32_t n, uint32_t len, int device, void *out) try {
    if (op != SIGN_PROBE_SHA512 && op != SIGN_PROBE_MOD_L && op != SIGN_PROBE_MULADD_MOD_E) return jfail(ZK_ERR_ARG, "unknown signer probe op");
    if (n == 0) return ZK_OK;
    const size_t ab = op == SIGN_PROBE_SHA512 ? (size_t)n * len : op == SIGN_PROBE_MOD_L ? sizeof(wide) * (size_t)n : sizeof(fe) * (size_t)n;
    const size_t bb = op == SIGN_PROBE_MULADD_MOD_E ? sizeof(fe) * (size_t)n : 0, ob = (op == SIGN_PROBE_SHA512 ? sizeof(wide) : sizeof(fe)) * (size_t)n;
    if (!out || (ab && !a) || (bb && (!b || !c))) return jfail(ZK_ERR_ARG, "null argument");
    if (n > (1u << 20) || ab > ((size_t)1 << 30)) return jfail(ZK_ERR_ARG, "the probe takes at most 2^20 items and 2^30 bytes per call");
    ZK_TRY(jj_use_device(device));
    const size_t ab_al = align32(ab);
    DevBuf buf;
    ZK_TRY(buf.ensure(ab_al + 2 * bb + ob + 32));
    char *d = (char *)buf.p;
    char *dA = d, *dB = dA + ab_al, *dC = dB + bb, *dO = dC + bb;
    if (ab) ZK_HIP(hipMemcpy(dA, a, ab, hipMemcpyHostToDevice));
    if (bb) { ZK_HIP(hipMemcpy(dB, b, bb, hipMemcpyHostToDevice)); ZK_HIP(hipMemcpy(dC, c, bb, hipMemcpyHostToDevice)); }
    ZK_LAUNCH(k_eddsa_sign_probe, zk_div_up(n, BLOCK), BLOCK, nullptr, op, (const void *)dA, (const fe *)dB, (const fe *)dC, n, len, (uint32_t *)dO);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, dO, ob, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD
