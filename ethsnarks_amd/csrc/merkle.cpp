// merkle.cpp -- the device Merkle tree behind zk_mtree_* (include/zkhip.h): storage, placeholders, launch structure.  Kernels: merkle.hpp.
//
// Launch structure.  An append of leaves s .. n - 1 re-hashes on level d + 1 the parents s >> (d + 1) .. cnt_{d+1} - 1.  Levels with more than
// TAIL_BLOCK such parents get one k_mimc_merkle_level launch each; every level above them runs inside ONE k_mimc_merkle_tail launch, so a
// bulk build costs (large levels + 1) hashing launches and a single append exactly one.  An update works the same way from the sorted,
// de-duplicated parent lists the host derives from the indices (k x depth integers).  ZK_MTREE_NO_TAIL=1 in the environment at creation makes
// a tree launch every level on its own instead: the form the tail kernel is measured against (profiles/merkle_tree.txt).
// zk_mtree_update_seq (ordered updates with transition witnesses) has the same split at k = TAIL_BLOCK updates: up to there ONE k_mtree_useq_tail
// launch walks every level, above (or with ZK_MTREE_NO_TAIL) every level is a k_mtree_useq_level launch; then the two witness launches and the commit.
// A tree over the Poseidon hasher (zk_mtree_create_ex; node width 2, 3 or 4) has the same launch structure with the k_poseidon_merkle_* kernels.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "bn254.hpp"
#include "merkle.hpp"
#include "poseidon.hpp"
#include "../../include/ethsnarks_hip/gadgets.hpp"              // the streaming sha256 and keccak256 (host code)
#include "../../include/zkhip.h"

using namespace zk;
using namespace zk::merkle;

static_assert(sizeof(zk_mtree_layout) == sizeof(Layout), "zk_mtree_layout and merkle::Layout are one struct");

namespace {
int mfail(int code, const char *msg) { return fail_msg(code, msg); }

int mt_use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return mfail(ZK_ERR_NODEVICE, "no HIP device (this library has no CPU path)");
    if (device < 0 || device >= n) return mfail(ZK_ERR_ARG, "device ordinal out of range");
    ZK_HIP(hipSetDevice(device));
    return ZK_OK;
}

// a 32-byte big-endian digest as a field element: value mod r, Montgomery (the Montgomery product by R^2 reduces any value < 2^256)
fe digest_to_mont(const uint8_t d[32]) {
    fe v;
    for (int i = 0; i < 8; i++) v.l[i] = ((uint32_t)d[28 - 4 * i] << 24) | ((uint32_t)d[29 - 4 * i] << 16) | ((uint32_t)d[30 - 4 * i] << 8) | d[31 - 4 * i];
    return Fr::to_mont(v);
}

// round constants: C_0 = keccak256(keccak256("mimc")), C_{i+1} = keccak256(C_i) (src/gadgets/mimc.hpp:260-290);
// IV_i = running sha256 of "MerkleTree-" || le16(i) (merkletree.py:36-44).  Montgomery; rc first, then iv.
struct Consts { fe rc[MIMC_ROUNDS]; fe iv[MAX_DEPTH]; };
const Consts &host_consts() {
    static Consts c;
    static std::once_flag once;
    std::call_once(once, [] {
        uint8_t dg[32], nx[32];
        ethsnarks::hashes::keccak256((const uint8_t *)"mimc", 4, dg);
        for (uint32_t i = 0; i < MIMC_ROUNDS; i++) {
            ethsnarks::hashes::keccak256(dg, 32, nx);
            memcpy(dg, nx, 32);
            c.rc[i] = digest_to_mont(dg);
        }
        ethsnarks::hashes::sha256 h;
        for (uint32_t i = 0; i < MAX_DEPTH; i++) {
            const uint8_t tag[13] = {'M', 'e', 'r', 'k', 'l', 'e', 'T', 'r', 'e', 'e', '-', (uint8_t)(i & 0xff), (uint8_t)(i >> 8)};
            h.update(tag, sizeof(tag));
            h.digest(dg);
            c.iv[i] = digest_to_mont(dg);
        }
    });
    return c;
}

// Poseidon (poseidon.hpp): C_i and the c of the Cauchy matrix M[i][j] = 1 / (c_i - c_{6+j}) are blake2b-256 chains -- the seed is hashed, then
// the raw 32-byte digest again and again; each digest read little-endian and reduced mod r, the reduction never feeding back into the chain
// (ethsnarks/poseidon/permutation.py:94-117, src/gadgets/poseidon.hpp:66-108).  Montgomery, canonical; C first, then M row major.
struct PConsts { fe c[poseidon::ROUNDS]; fe m[poseidon::T * poseidon::T]; };
static_assert(sizeof(PConsts) == sizeof(fe) * poseidon::N_CONSTS, "the device table is C then M");
void poseidon_chain(const char *seed, uint32_t n, fe *out) {
    uint8_t dg[32], nx[32];
    ethsnarks::hashes::blake2b((const uint8_t *)seed, strlen(seed), dg);
    for (uint32_t i = 0; i < n; i++) {
        fe v;
        for (int k = 0; k < 8; k++) v.l[k] = (uint32_t)dg[4 * k] | ((uint32_t)dg[4 * k + 1] << 8) | ((uint32_t)dg[4 * k + 2] << 16) | ((uint32_t)dg[4 * k + 3] << 24);
        out[i] = Fr::to_mont(v);                                // (the Montgomery product by R^2 reduces any value < 2^256)
        ethsnarks::hashes::blake2b(dg, 32, nx);
        memcpy(dg, nx, 32);
    }
}
const PConsts &host_pconsts() {
    static PConsts c;
    static std::once_flag once;
    std::call_once(once, [] {
        poseidon_chain("poseidon_constants", poseidon::ROUNDS, c.c);
        fe x[2 * poseidon::T];
        poseidon_chain("poseidon_matrix_0000", 2 * poseidon::T, x);
        for (uint32_t i = 0; i < poseidon::T; i++)
            for (uint32_t j = 0; j < poseidon::T; j++) c.m[poseidon::T * i + j] = Fr::inv(Fr::sub(x[i], x[poseidon::T + j]));
    });
    return c;
}

// unique(d, index) = sha256(be16(d) || be240(index)) mod r, Montgomery
fe placeholder(uint32_t d, uint64_t index) {
    uint8_t msg[32] = {0}, dg[32];
    msg[0] = (uint8_t)(d >> 8); msg[1] = (uint8_t)d;
    for (int k = 0; k < 8; k++) msg[31 - k] = (uint8_t)(index >> (8 * k));
    ethsnarks::hashes::sha256 h;
    h.update(msg, 32);
    h.digest(dg);
    return digest_to_mont(dg);
}

bool all_below_modulus(const uint64_t *v, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) { fe x; memcpy(x.l, v + 4 * i, 32); if (!fr_lt_modulus(x)) return false; }
    return true;
}
}  // namespace

struct zk_mtree {
    int device = 0;
    uint32_t depth = 0, width = 2;
    int hasher = ZK_MTREE_HASH_MIMC;
    uint64_t n = 0;                                             // leaves
    bool use_tail = true;
    hipStream_t st = nullptr;
    fe *lvl[MAX_DEPTH + 1] = {nullptr};                         // level d: cap[d] elements, level_count(n, d) of them in use
    uint64_t cap[MAX_DEPTH + 1] = {0};
    fe **d_lvl = nullptr;                                       // the pointers above, for the kernels
    fe *d_consts = nullptr;                                     // Consts
    fe *d_pconsts = nullptr;                                    // PConsts (Poseidon trees only)
    fe *d_ph = nullptr;                                         // MAX_DEPTH x (width - 1) placeholders: unique(d, count(d) + k)
    uint32_t *d_bad = nullptr;
    void *d_scratch = nullptr; size_t scratch_cap = 0;          // indices, lists, gathered paths: grows, never shrinks
    ~zk_mtree() {
        for (fe *p : lvl) if (p) (void)hipFree(p);
        void *bufs[] = {d_lvl, d_consts, d_pconsts, d_ph, d_bad, d_scratch};
        for (void *b : bufs) if (b) (void)hipFree(b);
        if (st) (void)hipStreamDestroy(st);
    }
    uint64_t level_cap_max(uint32_t d) const { return pow_w(width, depth - d); }
    uint64_t count(uint64_t leaves, uint32_t d) const { return level_count_w(leaves, d, width); }
    bool is_poseidon() const { return hasher == ZK_MTREE_HASH_POSEIDON; }
    TreeView view() const {
        TreeView v;
        v.lvl = d_lvl; v.ph = d_ph; v.rc = d_consts; v.iv = d_consts + MIMC_ROUNDS; v.pc = d_pconsts; v.n = n; v.depth = depth; v.width = width;
        return v;
    }
};

namespace {
int mt_scratch(zk_mtree *t, size_t bytes) {
    if (bytes <= t->scratch_cap) return ZK_OK;
    void *p = nullptr;
    const size_t want = std::max(bytes, 2 * t->scratch_cap);
    if (hipMalloc(&p, want) != hipSuccess) return mfail(ZK_ERR_NOMEM, "device allocation failed (Merkle tree scratch)");
    if (t->d_scratch) (void)hipFree(t->d_scratch);
    t->d_scratch = p; t->scratch_cap = want;
    return ZK_OK;
}

// placeholders for a tree of n_new leaves, queued on the stream (before the kernels that read them)
int mt_put_placeholders(zk_mtree *t, uint64_t n_new) {
    fe ph[MAX_DEPTH * (MAX_WIDTH - 1)];
    const uint32_t per = t->width - 1;
    for (uint32_t d = 0; d < MAX_DEPTH; d++)
        for (uint32_t k = 0; k < per; k++) ph[d * per + k] = d < t->depth ? placeholder(d, t->count(n_new, d) + k) : Fr::zero();
    for (uint32_t i = MAX_DEPTH * per; i < MAX_DEPTH * (MAX_WIDTH - 1); i++) ph[i] = Fr::zero();
    ZK_HIP(hipMemcpyAsync(t->d_ph, ph, sizeof(ph), hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipStreamSynchronize(t->st));                        // (ph lives on this stack frame)
    return ZK_OK;
}

// room for n_new leaves on every level: all new buffers are claimed before one is put in place, so a failure changes nothing
int mt_grow(zk_mtree *t, uint64_t n_new) {
    fe *fresh[MAX_DEPTH + 1] = {nullptr};
    uint64_t fresh_cap[MAX_DEPTH + 1] = {0};
    bool any = false;
    for (uint32_t d = 0; d <= t->depth; d++) {
        const uint64_t need = t->count(n_new, d);
        if (need <= t->cap[d]) continue;
        const uint64_t want = std::min(std::max(need, 2 * t->cap[d]), t->level_cap_max(d));
        if (hipMalloc(&fresh[d], sizeof(fe) * want) != hipSuccess) {
            for (uint32_t e = 0; e < d; e++) if (fresh[e]) (void)hipFree(fresh[e]);
            (void)hipGetLastError();
            return mfail(ZK_ERR_NOMEM, "device allocation failed (Merkle tree nodes)");
        }
        fresh_cap[d] = want; any = true;
    }
    if (!any) return ZK_OK;
    for (uint32_t d = 0; d <= t->depth; d++) {
        if (!fresh[d]) continue;
        const uint64_t used = t->count(t->n, d);
        if (used) ZK_HIP(hipMemcpyAsync(fresh[d], t->lvl[d], sizeof(fe) * used, hipMemcpyDeviceToDevice, t->st));
    }
    ZK_HIP(hipStreamSynchronize(t->st));
    for (uint32_t d = 0; d <= t->depth; d++) {
        if (!fresh[d]) continue;
        if (t->lvl[d]) (void)hipFree(t->lvl[d]);
        t->lvl[d] = fresh[d]; t->cap[d] = fresh_cap[d];
    }
    ZK_HIP(hipMemcpy(t->d_lvl, t->lvl, sizeof(t->lvl), hipMemcpyHostToDevice));
    return ZK_OK;
}

// hash the ancestors of the leaves s_old .. t->n - 1 (t->n already counts them, the placeholders are in place)
int mt_hash_appended(zk_mtree *t, uint64_t s_old) {
    const TreeView v = t->view();
    uint32_t d = 0;
    for (; d < t->depth; d++) {
        const uint64_t j0 = s_old / pow_w(t->width, d + 1), nj = t->count(t->n, d + 1) - j0;
        if (t->use_tail && nj <= TAIL_BLOCK) break;
        if (t->is_poseidon()) ZK_LAUNCH(k_poseidon_merkle_level, zk_div_up(nj, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d, j0, nj);
        else ZK_LAUNCH(k_mimc_merkle_level, zk_div_up(nj, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d, j0, nj);
    }
    if (d < t->depth) {
        if (t->is_poseidon()) ZK_LAUNCH_SYNC(k_poseidon_merkle_tail, 1, TAIL_BLOCK, t->st, v, d, s_old, (const uint64_t *)nullptr, (const uint32_t *)nullptr, 0u);
        else ZK_LAUNCH_SYNC(k_mimc_merkle_tail, 1, TAIL_BLOCK, t->st, v, d, s_old, (const uint64_t *)nullptr, (const uint32_t *)nullptr, 0u);
    }
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// leaves: host pointer (checked by the caller) or device pointer
int mt_append(zk_mtree *t, const void *src, bool resident, uint64_t n, int canonical) {
    if (n == 0) return ZK_OK;
    if (n > t->level_cap_max(0) - t->n) return mfail(ZK_ERR_ARG, "the tree is full: more leaves than width^depth");
    ZK_TRY(mt_use_device(t->device));
    const uint64_t s_old = t->n, n_new = s_old + n;
    ZK_TRY(mt_grow(t, n_new));
    fe *dst = t->lvl[0] + s_old;                                // slots past the size: a failure below leaves nothing to undo
    ZK_HIP(hipMemcpyAsync(dst, src, sizeof(fe) * n, resident ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, t->st));
    if (resident || canonical) {
        ZK_HIP(hipMemsetAsync(t->d_bad, 0, 4, t->st));
        ZK_LAUNCH(k_mtree_ingest, zk_div_up(n, LEVEL_BLOCK), LEVEL_BLOCK, t->st, dst, n, canonical, t->d_bad);
        ZK_HIP(hipGetLastError());
        if (resident) {
            uint32_t bad = 0;
            ZK_HIP(hipMemcpyAsync(&bad, t->d_bad, 4, hipMemcpyDeviceToHost, t->st));
            ZK_HIP(hipStreamSynchronize(t->st));
            if (bad) return mfail(ZK_ERR_ARG, "a leaf is not below the Fr modulus");
        }
    }
    ZK_TRY(mt_put_placeholders(t, n_new));
    t->n = n_new;
    ZK_TRY(mt_hash_appended(t, s_old));
    ZK_HIP(hipStreamSynchronize(t->st));
    return ZK_OK;
}

int mt_upload_indices(zk_mtree *t, const uint64_t *indices, uint32_t k, size_t extra_bytes) {
    for (uint32_t i = 0; i < k; i++) if (indices[i] >= t->n) return mfail(ZK_ERR_ARG, "leaf index is not below the size of the tree");
    ZK_TRY(mt_use_device(t->device));
    ZK_TRY(mt_scratch(t, sizeof(uint64_t) * (size_t)k + extra_bytes));
    ZK_HIP(hipMemcpyAsync(t->d_scratch, indices, sizeof(uint64_t) * (size_t)k, hipMemcpyHostToDevice, t->st));
    return ZK_OK;
}
}  // namespace

extern "C" int zk_mtree_create_ex(uint32_t depth, uint32_t width, int hasher, uint64_t reserve_leaves, int device, zk_mtree **out) try {
    if (!out) return mfail(ZK_ERR_ARG, "null argument");
    *out = nullptr;
    if (hasher != ZK_MTREE_HASH_MIMC && hasher != ZK_MTREE_HASH_POSEIDON) return mfail(ZK_ERR_ARG, "unknown hasher");
    if (hasher == ZK_MTREE_HASH_MIMC && width != 2) return mfail(ZK_ERR_ARG, "the MiMC tree has node width 2");
    if (width < 2 || width > MAX_WIDTH) return mfail(ZK_ERR_ARG, "the Poseidon tree has node width 2, 3 or 4");
    if (depth < 1 || depth > MAX_DEPTH) return mfail(ZK_ERR_ARG, "depth must be in 1 .. 29");
    if (hasher == ZK_MTREE_HASH_POSEIDON && depth > (width == 2 ? 29u : width == 3 ? 18u : 14u))
        return mfail(ZK_ERR_ARG, "a Poseidon tree holds at most 2^29 leaves: depth <= 29, 18, 14 at width 2, 3, 4");
    ZK_TRY(mt_use_device(device));
    std::unique_ptr<zk_mtree> t(new zk_mtree());
    t->device = device; t->depth = depth; t->width = width; t->hasher = hasher;
    if (const char *e = getenv("ZK_MTREE_NO_TAIL")) t->use_tail = !(e[0] == '1');
    ZK_HIP(hipStreamCreateWithFlags(&t->st, hipStreamNonBlocking));
    const Consts &c = host_consts();
    if (hipMalloc(&t->d_consts, sizeof(Consts)) != hipSuccess || (t->is_poseidon() && hipMalloc(&t->d_pconsts, sizeof(PConsts)) != hipSuccess) ||
        hipMalloc(&t->d_ph, sizeof(fe) * MAX_DEPTH * (MAX_WIDTH - 1)) != hipSuccess ||
        hipMalloc(&t->d_lvl, sizeof(t->lvl)) != hipSuccess || hipMalloc(&t->d_bad, 4) != hipSuccess)
        return mfail(ZK_ERR_NOMEM, "device allocation failed (Merkle tree)");
    ZK_HIP(hipMemcpy(t->d_consts, &c, sizeof(Consts), hipMemcpyHostToDevice));
    if (t->is_poseidon()) ZK_HIP(hipMemcpy(t->d_pconsts, &host_pconsts(), sizeof(PConsts), hipMemcpyHostToDevice));   // (a MiMC tree has no use for them)
    ZK_TRY(mt_grow(t.get(), std::max<uint64_t>(1, std::min(reserve_leaves, t->level_cap_max(0)))));
    ZK_TRY(mt_put_placeholders(t.get(), 0));
    *out = t.release();
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mtree_create(uint32_t depth, uint64_t reserve_leaves, int device, zk_mtree **out) {
    return zk_mtree_create_ex(depth, 2, ZK_MTREE_HASH_MIMC, reserve_leaves, device, out);
}

extern "C" int zk_mtree_info(const zk_mtree *t, uint32_t *depth, uint32_t *width, int *hasher) try {
    if (!t) return mfail(ZK_ERR_ARG, "null argument");
    if (depth) *depth = t->depth;
    if (width) *width = t->width;
    if (hasher) *hasher = t->hasher;
    return ZK_OK;
} ZK_GUARD

extern "C" void zk_mtree_free(zk_mtree *t) try {
    if (!t) return;
    (void)mt_use_device(t->device);
    delete t;
} ZK_GUARD_VOID

extern "C" int zk_mtree_size(const zk_mtree *t, uint64_t *n_leaves) try {
    if (!t || !n_leaves) return mfail(ZK_ERR_ARG, "null argument");
    *n_leaves = t->n;
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mtree_append(zk_mtree *t, const uint64_t *leaves, uint64_t n, int canonical) try {
    if (!t || (n && !leaves)) return mfail(ZK_ERR_ARG, "null argument");
    if (n > t->level_cap_max(0) - t->n) return mfail(ZK_ERR_ARG, "the tree is full: more leaves than width^depth");
    if (!all_below_modulus(leaves, n)) return mfail(ZK_ERR_ARG, "a leaf is not below the Fr modulus");
    return mt_append(t, leaves, false, n, canonical);
} ZK_GUARD

extern "C" int zk_mtree_append_resident(zk_mtree *t, const void *d_leaves, uint64_t n, int canonical) try {
    if (!t || (n && !d_leaves)) return mfail(ZK_ERR_ARG, "null argument");
    return mt_append(t, d_leaves, true, n, canonical);
} ZK_GUARD

extern "C" int zk_mtree_update(zk_mtree *t, const uint64_t *indices, const uint64_t *leaves, uint32_t k, int canonical) try {
    if (!t || (k && (!indices || !leaves))) return mfail(ZK_ERR_ARG, "null argument");
    if (k == 0) return ZK_OK;
    for (uint32_t i = 0; i < k; i++) if (indices[i] >= t->n) return mfail(ZK_ERR_ARG, "leaf index is not below the size of the tree");
    if (!all_below_modulus(leaves, k)) return mfail(ZK_ERR_ARG, "a leaf is not below the Fr modulus");
    // distinct indices in ascending order, each with the value of its last occurrence
    std::vector<uint32_t> order(k);
    for (uint32_t i = 0; i < k; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return indices[a] < indices[b]; });
    std::vector<uint64_t> idx; std::vector<fe> vals;
    idx.reserve(k); vals.reserve(k);
    for (uint32_t i = 0; i < k; i++) {
        if (i + 1 < k && indices[order[i + 1]] == indices[order[i]]) continue;
        fe v; memcpy(v.l, leaves + 4 * (size_t)order[i], 32);
        idx.push_back(indices[order[i]]); vals.push_back(canonical ? Fr::to_mont(v) : v);
    }
    const uint32_t m = (uint32_t)idx.size(), D = t->depth;
    // row d: the parents on level d + 1, sorted and distinct (a shift keeps the order)
    std::vector<uint64_t> lists((size_t)D * m);
    uint32_t nlist[MAX_DEPTH] = {0};
    std::vector<uint64_t> cur(idx);
    for (uint32_t d = 0; d < D; d++) {
        for (auto &j : cur) j /= t->width;
        cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
        nlist[d] = (uint32_t)cur.size();
        std::copy(cur.begin(), cur.end(), lists.begin() + (size_t)d * m);
    }
    ZK_TRY(mt_use_device(t->device));
    // scratch: idx | lists | nlist | vals
    const size_t o_lists = sizeof(uint64_t) * m, o_nlist = o_lists + sizeof(uint64_t) * (size_t)D * m, o_vals = (o_nlist + sizeof(nlist) + 31) & ~(size_t)31;
    ZK_TRY(mt_scratch(t, o_vals + sizeof(fe) * m));
    char *s = (char *)t->d_scratch;
    ZK_HIP(hipMemcpyAsync(s, idx.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipMemcpyAsync(s + o_lists, lists.data(), sizeof(uint64_t) * (size_t)D * m, hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipMemcpyAsync(s + o_nlist, nlist, sizeof(nlist), hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipMemcpyAsync(s + o_vals, vals.data(), sizeof(fe) * m, hipMemcpyHostToDevice, t->st));
    const TreeView v = t->view();
    ZK_LAUNCH(k_mtree_set_leaves, zk_div_up(m, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, (const uint64_t *)s, (const fe *)(s + o_vals), m);
    uint32_t d = 0;
    for (; d < D; d++) {
        if (t->use_tail && nlist[d] <= TAIL_BLOCK) break;
        if (t->is_poseidon()) ZK_LAUNCH(k_poseidon_merkle_update, zk_div_up(nlist[d], LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d, (const uint64_t *)(s + o_lists) + (size_t)d * m, nlist[d]);
        else ZK_LAUNCH(k_mimc_merkle_update, zk_div_up(nlist[d], LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d, (const uint64_t *)(s + o_lists) + (size_t)d * m, nlist[d]);
    }
    if (d < D) {
        if (t->is_poseidon()) ZK_LAUNCH_SYNC(k_poseidon_merkle_tail, 1, TAIL_BLOCK, t->st, v, d, (uint64_t)0, (const uint64_t *)(s + o_lists), (const uint32_t *)(s + o_nlist), m);
        else ZK_LAUNCH_SYNC(k_mimc_merkle_tail, 1, TAIL_BLOCK, t->st, v, d, (uint64_t)0, (const uint64_t *)(s + o_lists), (const uint32_t *)(s + o_nlist), m);
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(t->st));                        // (the staging vectors live until here)
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mtree_node(const zk_mtree *t, uint32_t level, uint64_t offset, uint64_t out_canon[4]) try {
    if (!t || !out_canon) return mfail(ZK_ERR_ARG, "null argument");
    if (level > t->depth || offset >= t->level_cap_max(level)) return mfail(ZK_ERR_ARG, "no such node: level <= depth and offset < width^(depth - level)");
    fe v;
    if (offset < t->count(t->n, level)) {
        ZK_TRY(mt_use_device(t->device));
        ZK_HIP(hipMemcpy(&v, t->lvl[level] + offset, sizeof(fe), hipMemcpyDeviceToHost));
    } else v = placeholder(level, offset);
    v = Fr::from_mont(v);
    memcpy(out_canon, v.l, 32);
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mtree_root(const zk_mtree *t, uint64_t root_canon[4]) try {
    if (!t || !root_canon) return mfail(ZK_ERR_ARG, "null argument");
    if (t->n == 0) return mfail(ZK_ERR_ARG, "the tree is empty: it has no root");
    return zk_mtree_node(t, t->depth, 0, root_canon);
} ZK_GUARD

extern "C" int zk_mtree_paths(const zk_mtree *ct, const uint64_t *indices, uint32_t k, uint64_t *leaves_canon, uint64_t *paths_canon) try {
    zk_mtree *t = const_cast<zk_mtree *>(ct);                   // (the stream and the scratch buffer; the tree itself is only read)
    if (!t || (k && !indices)) return mfail(ZK_ERR_ARG, "null argument");
    if (k == 0) return ZK_OK;
    const size_t per = (size_t)t->depth * (t->width - 1);      // siblings of one path
    const size_t o_leaves = (sizeof(uint64_t) * (size_t)k + 31) & ~(size_t)31, o_paths = o_leaves + sizeof(fe) * (size_t)k;
    ZK_TRY(mt_upload_indices(t, indices, k, o_paths + sizeof(fe) * (size_t)k * per));
    char *s = (char *)t->d_scratch;
    ZK_LAUNCH(k_mtree_gather, zk_div_up((uint64_t)k * (per + 1), LEVEL_BLOCK), LEVEL_BLOCK, t->st, t->view(), (const uint64_t *)s, k, (fe *)(s + o_leaves), (fe *)(s + o_paths));
    ZK_HIP(hipGetLastError());
    if (leaves_canon) ZK_HIP(hipMemcpyAsync(leaves_canon, s + o_leaves, sizeof(fe) * (size_t)k, hipMemcpyDeviceToHost, t->st));
    if (paths_canon) ZK_HIP(hipMemcpyAsync(paths_canon, s + o_paths, sizeof(fe) * (size_t)k * per, hipMemcpyDeviceToHost, t->st));
    ZK_HIP(hipStreamSynchronize(t->st));
    return ZK_OK;
} ZK_GUARD

namespace {
// the checks of a membership layout that both fill calls make, before any device work
int mt_check_layout(const zk_mtree *t, uint64_t row_elems, const zk_mtree_layout *layout) {
    const uint64_t D = t->depth;
    if (t->is_poseidon() && layout->n_iv != 0) return mfail(ZK_ERR_ARG, "the Poseidon membership circuit has no IV variables: layout.n_iv must be 0");
    if (layout->n_iv > MAX_DEPTH || row_elems == 0 || layout->root_var >= row_elems || layout->leaf_var >= row_elems || layout->addr_var0 + D > row_elems ||
        layout->path_var0 + D > row_elems || (uint64_t)layout->iv_var0 + layout->n_iv > row_elems)
        return mfail(ZK_ERR_ARG, "the layout names a variable outside the witness row");
    return ZK_OK;
}
}  // namespace

extern "C" int zk_mtree_fill_witnesses(const zk_mtree *ct, const uint64_t *indices, uint32_t k, void *d_w, uint64_t row_elems, const zk_mtree_layout *layout) try {
    zk_mtree *t = const_cast<zk_mtree *>(ct);
    if (!t || (k && !indices) || !d_w || !layout) return mfail(ZK_ERR_ARG, "null argument");
    if (t->width != 2) return mfail(ZK_ERR_ARG, "the membership circuit exists for node width 2 only (there is no wide path selector)");
    if (k == 0) return ZK_OK;
    if (t->n == 0) return mfail(ZK_ERR_ARG, "the tree is empty: it has no root");
    const uint64_t D = t->depth;
    ZK_TRY(mt_check_layout(t, row_elems, layout));
    ZK_TRY(mt_upload_indices(t, indices, k, 0));
    Layout L;
    memcpy(&L, layout, sizeof(L));
    ZK_LAUNCH(k_mtree_fill_witness, zk_div_up((uint64_t)k * (3 + 2 * D + L.n_iv), LEVEL_BLOCK), LEVEL_BLOCK, t->st, t->view(), (const uint64_t *)t->d_scratch, k, (fe *)d_w, row_elems, L);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(t->st));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mtree_fill_full_witnesses(const zk_mtree *ct, const uint64_t *indices, uint32_t k, void *d_w, uint64_t row_elems, const zk_mtree_layout *layout,
                                            uint32_t level_var0, uint32_t level_stride) try {
    zk_mtree *t = const_cast<zk_mtree *>(ct);
    if (!t || (k && !indices) || !d_w || !layout) return mfail(ZK_ERR_ARG, "null argument");
    if (t->width != 2) return mfail(ZK_ERR_ARG, "the membership circuit exists for node width 2 only (there is no wide path selector)");
    if (k == 0) return ZK_OK;
    if (t->n == 0) return mfail(ZK_ERR_ARG, "the tree is empty: it has no root");
    const uint64_t D = t->depth;
    ZK_TRY(mt_check_layout(t, row_elems, layout));
    if (!t->is_poseidon() && layout->n_iv < D) return mfail(ZK_ERR_ARG, "a complete MiMC witness reads the level IVs: layout.n_iv must be at least the depth");
    if (level_stride < (t->is_poseidon() ? POSEIDON_LEVEL_VARS : MIMC_LEVEL_VARS))
        return mfail(ZK_ERR_ARG, "level_stride is below the variables of one level: 322 (Poseidon) or 736 (MiMC)");
    const uint64_t lv0 = level_var0, lv1 = lv0 + D * level_stride;                         // the level blocks: [lv0, lv1)
    if (lv1 > row_elems) return mfail(ZK_ERR_ARG, "the level blocks leave the witness row: level_var0 + depth * level_stride > row_elems");
    const auto hits = [&](uint64_t v0, uint64_t n) { return n && v0 < lv1 && v0 + n > lv0; };
    if (hits(0, 1) || hits(layout->root_var, 1) || hits(layout->leaf_var, 1) || hits(layout->addr_var0, D) || hits(layout->path_var0, D) || hits(layout->iv_var0, layout->n_iv))
        return mfail(ZK_ERR_ARG, "the level blocks overlap an input variable of the layout");
    ZK_TRY(mt_upload_indices(t, indices, k, 0));
    Layout L;
    memcpy(&L, layout, sizeof(L));
    const TreeView v = t->view();
    const uint64_t *d_idx = (const uint64_t *)t->d_scratch;
    ZK_LAUNCH(k_mtree_fill_witness, zk_div_up((uint64_t)k * (3 + 2 * D + L.n_iv), LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d_idx, k, (fe *)d_w, row_elems, L);
    if (t->is_poseidon()) ZK_LAUNCH(k_mtree_fill_levels<true>, zk_div_up((uint64_t)k * D, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d_idx, k, (fe *)d_w, row_elems, level_var0, level_stride);
    else ZK_LAUNCH(k_mtree_fill_levels<false>, zk_div_up((uint64_t)k * D, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, d_idx, k, (fe *)d_w, row_elems, level_var0, level_stride);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(t->st));
    return ZK_OK;
} ZK_GUARD

// ---- ordered updates with transition witnesses (kernels and notation: merkle.hpp, "ordered leaf updates")
static_assert(sizeof(zk_mtree_update_layout) == sizeof(UpdateLayout), "zk_mtree_update_layout and merkle::UpdateLayout are one struct");

namespace {
// node -> the last update seen on it, for one level at a time: open addressing over 2^b >= 2 k slots, emptied between levels
struct LastSeen {
    std::vector<uint64_t> key;
    std::vector<int32_t> val;
    uint32_t shift = 63;
    explicit LastSeen(uint32_t k) { size_t n = 2; while (n < 2 * (size_t)k) { n *= 2; shift--; } key.resize(n); val.resize(n); }
    void clear() { std::fill(val.begin(), val.end(), -1); }
    int32_t &at(uint64_t node) {                                // the slot of `node`: -1 while no update has touched it
        size_t h = (size_t)((node * 0x9E3779B97F4A7C15ull) >> shift);
        while (val[h] >= 0 && key[h] != node) h = (h + 1) & (key.size() - 1);
        key[h] = node;
        return val[h];
    }
};

// one ordered pass per level, O(k D): pred_same / pred_sib (D x k) and last ((D + 1) x k) of merkle::UpdateSeq
void useq_predecessors(const uint64_t *indices, uint32_t k, uint32_t D, int32_t *pred_same, int32_t *pred_sib, uint8_t *last) {
    LastSeen seen(k);
    for (uint32_t d = 0; d <= D; d++) {
        seen.clear();
        for (uint32_t j = 0; j < k; j++) {
            const uint64_t node = indices[j] >> d;
            const int32_t sib = seen.at(node ^ 1);
            int32_t &same = seen.at(node);
            if (d < D) { pred_same[(size_t)d * k + j] = same; pred_sib[(size_t)d * k + j] = sib; }
            if (same >= 0) last[(size_t)d * k + same] = 0;
            last[(size_t)d * k + j] = 1;
            same = (int32_t)j;
        }
    }
}

double ms_since(const struct timespec &t0) {
    struct timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    return 1e3 * (double)(t1.tv_sec - t0.tv_sec) + 1e-6 * (double)(t1.tv_nsec - t0.tv_nsec);
}
}  // namespace

extern "C" int zk_mtree_update_seq(zk_mtree *t, const uint64_t *indices, const uint64_t *leaves, uint32_t k, int canonical, void *d_w, uint64_t row_elems,
                                   const zk_mtree_update_layout *layout, uint32_t level_var0, uint32_t level_stride, uint64_t *roots_canon) try {
    if (!t || (k && (!indices || !leaves)) || (d_w && !layout)) return mfail(ZK_ERR_ARG, "null argument");
    if (t->width != 2) return mfail(ZK_ERR_ARG, "the update circuit exists for node width 2 only (there is no wide path selector)");
    if (t->n == 0) return mfail(ZK_ERR_ARG, "the tree is empty: it has no root and no leaf to update");
    if (k > 0x7fffffffu) return mfail(ZK_ERR_ARG, "more than 2^31 - 1 updates in one call");
    const uint32_t D = t->depth;
    for (uint32_t i = 0; i < k; i++) if (indices[i] >= t->n) return mfail(ZK_ERR_ARG, "leaf index is not below the size of the tree");
    if (!all_below_modulus(leaves, k)) return mfail(ZK_ERR_ARG, "a leaf is not below the Fr modulus");
    UpdateLayout L = {};
    if (d_w) {
        memcpy(&L, layout, sizeof(L));
        if (t->is_poseidon() && L.n_iv != 0) return mfail(ZK_ERR_ARG, "the Poseidon update circuit has no IV variables: layout.n_iv must be 0");
        if (!t->is_poseidon() && L.n_iv < D) return mfail(ZK_ERR_ARG, "a complete MiMC witness reads the level IVs: layout.n_iv must be at least the depth");
        if (L.n_iv > MAX_DEPTH || row_elems == 0 || L.old_root_var >= row_elems || L.new_root_var >= row_elems || L.old_leaf_var >= row_elems || L.new_leaf_var >= row_elems ||
            (uint64_t)L.addr_var0 + D > row_elems || (uint64_t)L.path_var0 + D > row_elems || (uint64_t)L.iv_var0 + L.n_iv > row_elems)
            return mfail(ZK_ERR_ARG, "the layout names a variable outside the witness row");
        if (level_stride < (t->is_poseidon() ? POSEIDON_LEVEL_VARS : MIMC_LEVEL_VARS))
            return mfail(ZK_ERR_ARG, "level_stride is below the variables of one level: 322 (Poseidon) or 736 (MiMC)");
        const uint64_t lv0 = level_var0, lv1 = lv0 + 2 * (uint64_t)D * level_stride;       // the level blocks of both chains: [lv0, lv1)
        if (lv1 > row_elems) return mfail(ZK_ERR_ARG, "the level blocks leave the witness row: level_var0 + 2 * depth * level_stride > row_elems");
        const auto hits = [&](uint64_t v0, uint64_t n) { return n && v0 < lv1 && v0 + n > lv0; };
        if (hits(0, 1) || hits(L.old_root_var, 1) || hits(L.new_root_var, 1) || hits(L.old_leaf_var, 1) || hits(L.new_leaf_var, 1) || hits(L.addr_var0, D) ||
            hits(L.path_var0, D) || hits(L.iv_var0, L.n_iv))
            return mfail(ZK_ERR_ARG, "the level blocks overlap an input variable of the layout");
    }
    if (k == 0) return roots_canon ? zk_mtree_root(t, roots_canon) : ZK_OK;
    // host: the predecessor tables and the new leaves in Montgomery form.  MEASUREMENT ONLY: ZK_MTREE_USEQ_TIMING=1 in the environment makes the
    // call report the time of the predecessor pass on stderr (tools/merkle_update_bench.py reads it); otherwise no clock is read
    const char *e_timing = getenv("ZK_MTREE_USEQ_TIMING");
    const bool timing = e_timing && e_timing[0] == '1';
    struct timespec t_pred = {};
    if (timing) clock_gettime(CLOCK_MONOTONIC, &t_pred);
    std::vector<int32_t> pred(2 * (size_t)D * k);
    std::vector<uint8_t> last((size_t)(D + 1) * k);
    useq_predecessors(indices, k, D, pred.data(), pred.data() + (size_t)D * k, last.data());
    if (timing) fprintf(stderr, "zk_mtree_update_seq: k = %u, host predecessor pass %.4f ms\n", k, ms_since(t_pred));
    std::vector<fe> vals(k);
    for (uint32_t i = 0; i < k; i++) { fe v; memcpy(v.l, leaves + 4 * (size_t)i, 32); vals[i] = canonical ? Fr::to_mont(v) : v; }
    ZK_TRY(mt_use_device(t->device));
    // scratch: idx | pred_same | pred_sib | last | nodes
    const auto up32 = [](size_t o) { return (o + 31) & ~(size_t)31; };
    const size_t o_pred = sizeof(uint64_t) * (size_t)k, o_last = o_pred + sizeof(int32_t) * pred.size(), o_nodes = up32(o_last + last.size());
    ZK_TRY(mt_scratch(t, o_nodes + sizeof(fe) * (size_t)(D + 1) * k));
    char *s = (char *)t->d_scratch;
    UpdateSeq u;
    u.idx = (const uint64_t *)s; u.pred_same = (const int32_t *)(s + o_pred); u.pred_sib = u.pred_same + (size_t)D * k;
    u.last = (const uint8_t *)(s + o_last); u.nodes = (fe *)(s + o_nodes); u.k = k;
    ZK_HIP(hipMemcpyAsync(s, indices, sizeof(uint64_t) * (size_t)k, hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipMemcpyAsync(s + o_pred, pred.data(), sizeof(int32_t) * pred.size(), hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipMemcpyAsync(s + o_last, last.data(), last.size(), hipMemcpyHostToDevice, t->st));
    ZK_HIP(hipMemcpyAsync(u.nodes, vals.data(), sizeof(fe) * (size_t)k, hipMemcpyHostToDevice, t->st));
    std::vector<fe> roots(roots_canon ? (size_t)k + 1 : 0);
    if (roots_canon) ZK_HIP(hipMemcpyAsync(roots.data(), t->lvl[D], sizeof(fe), hipMemcpyDeviceToHost, t->st));     // (queued before the commit)
    const TreeView v = t->view();
    const bool pos = t->is_poseidon();
    // phase 1: D dependent steps
    if (t->use_tail && k <= TAIL_BLOCK) {
        if (pos) ZK_LAUNCH_SYNC(k_mtree_useq_tail<true>, 1, TAIL_BLOCK, t->st, v, u);
        else ZK_LAUNCH_SYNC(k_mtree_useq_tail<false>, 1, TAIL_BLOCK, t->st, v, u);
    } else for (uint32_t d = 0; d < D; d++) {
        if (pos) ZK_LAUNCH(k_mtree_useq_level<true>, zk_div_up(k, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, u, d);
        else ZK_LAUNCH(k_mtree_useq_level<false>, zk_div_up(k, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, u, d);
    }
    // phase 2: the witness rows
    if (d_w) {
        ZK_LAUNCH(k_mtree_useq_fill_inputs, zk_div_up((uint64_t)k * (5 + 2 * D + L.n_iv), LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, u, (fe *)d_w, row_elems, L);
        if (pos) ZK_LAUNCH(k_mtree_useq_fill_levels<true>, zk_div_up((uint64_t)k * D * 2, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, u, (fe *)d_w, row_elems, level_var0, level_stride);
        else ZK_LAUNCH(k_mtree_useq_fill_levels<false>, zk_div_up((uint64_t)k * D * 2, LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, u, (fe *)d_w, row_elems, level_var0, level_stride);
    }
    // phase 3: the only writes to the tree
    ZK_LAUNCH(k_mtree_useq_commit, zk_div_up((uint64_t)k * (D + 1), LEVEL_BLOCK), LEVEL_BLOCK, t->st, v, u);
    ZK_HIP(hipGetLastError());
    if (roots_canon) ZK_HIP(hipMemcpyAsync(roots.data() + 1, u.nodes + (size_t)D * k, sizeof(fe) * (size_t)k, hipMemcpyDeviceToHost, t->st));
    ZK_HIP(hipStreamSynchronize(t->st));                        // (the staging vectors live until here)
    for (size_t i = 0; i < roots.size(); i++) { const fe r = Fr::from_mont(roots[i]); memcpy(roots_canon + 4 * i, r.l, 32); }
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mimc_constants(uint64_t *round_constants_canon, uint64_t *ivs_canon) try {
    const Consts &c = host_consts();
    if (round_constants_canon) for (uint32_t i = 0; i < MIMC_ROUNDS; i++) { const fe v = Fr::from_mont(c.rc[i]); memcpy(round_constants_canon + 4 * i, v.l, 32); }
    if (ivs_canon) for (uint32_t i = 0; i < MAX_DEPTH; i++) { const fe v = Fr::from_mont(c.iv[i]); memcpy(ivs_canon + 4 * i, v.l, 32); }
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_mimc_hash2(const uint64_t *left, const uint64_t *right, const uint64_t *iv, uint32_t n, int device, uint64_t *out) try {
    if (!left || !right || !iv || !out) return mfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(left, n) || !all_below_modulus(right, n) || !all_below_modulus(iv, n)) return mfail(ZK_ERR_ARG, "an operand is not below the Fr modulus");
    ZK_TRY(mt_use_device(device));
    const Consts &c = host_consts();
    struct Buf { fe *p = nullptr; ~Buf() { if (p) (void)hipFree(p); } } in, rc;
    const size_t bytes = sizeof(fe) * (size_t)n;
    if (hipMalloc(&in.p, 4 * bytes) != hipSuccess || hipMalloc(&rc.p, sizeof(c.rc)) != hipSuccess) return mfail(ZK_ERR_NOMEM, "device allocation failed");
    ZK_HIP(hipMemcpy(in.p, left, bytes, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(in.p + n, right, bytes, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(in.p + 2 * (size_t)n, iv, bytes, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(rc.p, c.rc, sizeof(c.rc), hipMemcpyHostToDevice));
    ZK_LAUNCH(k_mimc_hash2, zk_div_up(n, LEVEL_BLOCK), LEVEL_BLOCK, nullptr, (const fe *)in.p, (const fe *)(in.p + n), (const fe *)(in.p + 2 * (size_t)n), n, (const fe *)rc.p, in.p + 3 * (size_t)n);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, in.p + 3 * (size_t)n, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

// ---- Poseidon by itself
extern "C" int zk_poseidon_constants(uint64_t *C_canon, uint64_t *M_canon) try {
    const PConsts &c = host_pconsts();
    if (C_canon) for (uint32_t i = 0; i < poseidon::ROUNDS; i++) { const fe v = Fr::from_mont(c.c[i]); memcpy(C_canon + 4 * i, v.l, 32); }
    if (M_canon) for (uint32_t i = 0; i < poseidon::T * poseidon::T; i++) { const fe v = Fr::from_mont(c.m[i]); memcpy(M_canon + 4 * i, v.l, 32); }
    return ZK_OK;
} ZK_GUARD

namespace {
// ZK_POSEIDON_MIX=lmul / dot6 in the environment picks the MIX form of zk_poseidon_hash and zk_poseidon_permute for a call: a TEST AND
// MEASUREMENT knob like ZK_MTREE_NO_TAIL (the two forms are tested and measured against each other, tests/test_poseidon_gpu.py,
// tools/poseidon_bench.py; documented in zkhip.h); unset or anything else: the form the tree uses.  The tree never reads it
bool poseidon_use_dot6() {
    const char *e = getenv("ZK_POSEIDON_MIX");
    if (e && !strcmp(e, "lmul")) return false;
    if (e && !strcmp(e, "dot6")) return true;
    return poseidon::POSEIDON_MIX_DOT6;
}
struct DevBuf { fe *p = nullptr; ~DevBuf() { if (p) (void)hipFree(p); } };
}  // namespace

extern "C" int zk_poseidon_hash(const uint64_t *inputs, uint32_t n_in, uint32_t n, int device, uint64_t *out) try {
    if (!inputs || !out) return mfail(ZK_ERR_ARG, "null argument");
    if (n_in < 1 || n_in >= poseidon::T) return mfail(ZK_ERR_ARG, "a hash takes 1 .. 5 inputs");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(inputs, (uint64_t)n * n_in)) return mfail(ZK_ERR_ARG, "an operand is not below the Fr modulus");
    ZK_TRY(mt_use_device(device));
    const PConsts &c = host_pconsts();
    DevBuf in, pc, o;
    if (hipMalloc(&in.p, sizeof(fe) * (size_t)n * n_in) != hipSuccess || hipMalloc(&pc.p, sizeof(PConsts)) != hipSuccess || hipMalloc(&o.p, sizeof(fe) * (size_t)n) != hipSuccess)
        return mfail(ZK_ERR_NOMEM, "device allocation failed");
    ZK_HIP(hipMemcpy(in.p, inputs, sizeof(fe) * (size_t)n * n_in, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(pc.p, &c, sizeof(PConsts), hipMemcpyHostToDevice));
    if (poseidon_use_dot6()) ZK_LAUNCH(poseidon::k_poseidon_hash<true>, zk_div_up(n, poseidon::BLOCK), poseidon::BLOCK, nullptr, (const fe *)in.p, n_in, n, (const fe *)pc.p, o.p);
    else ZK_LAUNCH(poseidon::k_poseidon_hash<false>, zk_div_up(n, poseidon::BLOCK), poseidon::BLOCK, nullptr, (const fe *)in.p, n_in, n, (const fe *)pc.p, o.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(out, o.p, sizeof(fe) * (size_t)n, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_poseidon_permute(uint64_t *states, uint32_t n, int device) try {
    if (!states) return mfail(ZK_ERR_ARG, "null argument");
    if (n == 0) return ZK_OK;
    if (!all_below_modulus(states, (uint64_t)n * poseidon::T)) return mfail(ZK_ERR_ARG, "an operand is not below the Fr modulus");
    ZK_TRY(mt_use_device(device));
    const PConsts &c = host_pconsts();
    DevBuf st, pc;
    const size_t bytes = sizeof(fe) * (size_t)n * poseidon::T;
    if (hipMalloc(&st.p, bytes) != hipSuccess || hipMalloc(&pc.p, sizeof(PConsts)) != hipSuccess) return mfail(ZK_ERR_NOMEM, "device allocation failed");
    ZK_HIP(hipMemcpy(st.p, states, bytes, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(pc.p, &c, sizeof(PConsts), hipMemcpyHostToDevice));
    if (poseidon_use_dot6()) ZK_LAUNCH(poseidon::k_poseidon_permute<true>, zk_div_up(n, poseidon::BLOCK), poseidon::BLOCK, nullptr, st.p, n, (const fe *)pc.p);
    else ZK_LAUNCH(poseidon::k_poseidon_permute<false>, zk_div_up(n, poseidon::BLOCK), poseidon::BLOCK, nullptr, st.p, n, (const fe *)pc.p);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    ZK_HIP(hipMemcpy(states, st.p, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD
