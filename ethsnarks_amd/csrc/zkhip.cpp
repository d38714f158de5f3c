// zkhip.cpp -- C ABI (include/zkhip.h) of the MI355X Groth16 proving backend.
// Compiled as HIP for gfx950 (see Makefile).  Host-side restatement of the reference's driver
//   r1cs_gg_ppzksnark_zok_prover   src/r1cs_gg_ppzksnark_zok/r1cs_gg_ppzksnark_zok.tcc:451-550
//   pk_nozk stream operators       ...tcc:108-143
//   proof_to_json                  src/export.cpp:20-121
// around the kernels of ntt.hpp / msm.hpp.  No CPU compute path exists in this library.
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>
#include <chrono>
#include <string.h>
#include <stddef.h>
#include <stdlib.h>
#include <sys/stat.h>

#include "common.hpp"
#include "bn254.hpp"
#include "ntt.hpp"
#include "msm.hpp"
#include "keygen.hpp"
#include "blind.hpp"
#include "hlagrange.hpp"
#include "../../include/zkhip.h"
#include <errno.h>
#include <sys/random.h>

namespace zk { thread_local char g_last_error[256] = ""; }
using namespace zk;

// the handler every extern "C" entry point ends in (common.hpp ZK_GUARD): called inside a catch (...) block
int zk::on_exception() noexcept {
    try { throw; }
    catch (const std::bad_alloc &) { return fail_msg(ZK_ERR_NOMEM, "out of host memory (std::bad_alloc)"); }
    catch (const std::length_error &e) { snprintf(g_last_error, sizeof(g_last_error), "out of host memory (std::length_error: %s)", e.what()); return ZK_ERR_NOMEM; }
    catch (const std::exception &e) { snprintf(g_last_error, sizeof(g_last_error), "internal error: %s", e.what()); return ZK_ERR_INTERNAL; }
    catch (...) { return fail_msg(ZK_ERR_INTERNAL, "internal error: unknown exception"); }
}

// ---- launch accounting (common.hpp: ZK_LAUNCH)
#ifndef ZK_EMUL
namespace {
std::atomic<uint64_t> g_launches{0};
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
struct ProfRec { const char *name; hipEvent_t e0, e1; };
std::vector<ProfRec> g_prof;
thread_local hipEvent_t t_pending = nullptr;
}  // namespace
void zk::launch_pre(const char *name, hipStream_t st) {
    g_launches.fetch_add(1, std::memory_order_relaxed);
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    ProfRec r{name, nullptr, nullptr};
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
    (void)hipEventRecord(r.e0, st);
    t_pending = r.e1;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(r);
}
void zk::launch_post(hipStream_t st) {
    if (t_pending) { (void)hipEventRecord(t_pending, st); t_pending = nullptr; }
}
extern "C" uint64_t zk_launch_count(void) { return g_launches.load(); }
#ifdef ZK_EXP_MARGINAL
// The launches of one bucket sort are producers and consumers of each other's buffers IN PLACE: k_sort_colscan scans the count matrix that
// k_sort_count wrote, k_sort_binscan / k_sort_partition / k_sort_fine read what the scans left.  Dropping a producer while its consumer still runs
// makes the consumer work on the previous proof's ALREADY SCANNED state -- round 3's "no sort_count,partition" experiment (variants/marg2.sh) let
// k_sort_colscan scan scanned counts a second time, k_sort_binscan turn the inflated bin totals into bin bases far beyond the entry count, and
// k_sort_fine then load `pairs[e]` (and store `sorted[...]`) at those bases, past the end of both allocations: a device fault, whose text the script
// had sent to /dev/null.  A skip list must therefore name ALL FIVE sort kernels or none; anything else is refused here (nothing is skipped, and
// the refusal is printed once), as is a list that drops k_msm_bucket_finalize / k_msm_heavy but keeps the accumulation they depend on being fresh
// -- that one is harmless (stale pieces of the same witness) and stays allowed.
static bool exp_list_has(const char *list, const char *name) {
    for (const char *p = list; *p;) {
        const char *e = strchr(p, ';'); const size_t n = e ? (size_t)(e - p) : strlen(p);
        if (n && std::string(name).find(std::string(p, n)) != std::string::npos) return true;
        p += n + (e ? 1 : 0);
    }
    return false;
}
bool zk::exp_skip(const char *name) {
    static const char *list = getenv("ZK_EXP_SKIP");
    static const uint64_t after = getenv("ZK_EXP_SKIP_AFTER") ? strtoull(getenv("ZK_EXP_SKIP_AFTER"), nullptr, 10) : 150;
    static const bool valid = [] {
        if (!list || !*list) return true;
        const char *chain[] = {"k_sort_count<C>", "k_sort_colscan<C>", "k_sort_binscan<C>", "k_sort_partition_staged<C>", "k_sort_partition<C>", "k_sort_fine<C>"};
        int hit = 0;
        for (const char *k : chain) hit += exp_list_has(list, k);
        if (hit != 0 && hit != 6) {
            fprintf(stderr, "zkhip (measurement build): ZK_EXP_SKIP=\"%s\" drops part of the bucket-sort chain: its kernels scan each other's buffers in place, "
                            "a consumer without its producer indexes past its allocations.  Name all of k_sort_ or none.  Nothing is skipped.\n", list);
            return false;
        }
        return true;
    }();
    if (!valid || !list || !*list || g_launches.load(std::memory_order_relaxed) < after) return false;
    return exp_list_has(list, name);
}
#endif
extern "C" int zk_profile_begin(void) try {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    g_prof.clear();
    g_prof_on = true;
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_profile_end(float *kernel_ms_sum, uint32_t *launches, char *buf, size_t cap) try {
    g_prof_on = false;
    if (hipDeviceSynchronize() != hipSuccess) return fail_msg(ZK_ERR_HIP, "hipDeviceSynchronize failed");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    float sum = 0;
    std::vector<std::pair<std::string, std::pair<float, uint32_t>>> by;      // name -> (ms, calls)
    for (auto &r : g_prof) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) ms = 0;
        sum += ms;
        bool found = false;
        for (auto &b : by) if (b.first == r.name) { b.second.first += ms; b.second.second++; found = true; break; }
        if (!found) by.push_back({r.name, {ms, 1u}});
        hipEventDestroy(r.e0); hipEventDestroy(r.e1);
    }
    if (kernel_ms_sum) *kernel_ms_sum = sum;
    if (launches) *launches = (uint32_t)g_prof.size();
    g_prof.clear();
    if (buf && cap) {                                     // "name calls ms" lines, longest first
        std::sort(by.begin(), by.end(), [](const auto &a, const auto &b) { return a.second.first > b.second.first; });
        std::string s;
        for (auto &b : by) { char line[256]; snprintf(line, sizeof(line), "%s %u %.4f\n", b.first.c_str(), b.second.second, b.second.first); s += line; }
        snprintf(buf, cap, "%s", s.c_str());
    }
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_device_info(int device, uint32_t *compute_units, uint32_t *clock_mhz, char *name, size_t name_cap) try {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return fail_msg(ZK_ERR_NODEVICE, "hipGetDeviceProperties failed: no usable HIP device");
    if (compute_units) *compute_units = (uint32_t)p.multiProcessorCount;
    if (clock_mhz) *clock_mhz = (uint32_t)(p.clockRate / 1000);
    if (name && name_cap) snprintf(name, name_cap, "%s", p.name);
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_device_pci_bus_id(int device, char *buf, size_t cap) try {
    if (!buf || cap < 16) return fail_msg(ZK_ERR_ARG, "buffer too small");
    if (hipDeviceGetPCIBusId(buf, (int)cap, device) != hipSuccess) return fail_msg(ZK_ERR_NODEVICE, "hipDeviceGetPCIBusId failed: no usable HIP device");
    return ZK_OK;
} ZK_GUARD
#else
extern "C" int zk_device_pci_bus_id(int, char *buf, size_t cap) try { if (buf && cap) snprintf(buf, cap, "emulation"); return ZK_OK; } ZK_GUARD
extern "C" uint64_t zk_launch_count(void) { return 0; }
extern "C" int zk_profile_begin(void) try { return ZK_OK; } ZK_GUARD
extern "C" int zk_profile_end(float *s, uint32_t *n, char *buf, size_t cap) try { if (s) *s = 0; if (n) *n = 0; if (buf && cap) buf[0] = 0; return ZK_OK; } ZK_GUARD
extern "C" int zk_device_info(int, uint32_t *cu, uint32_t *mhz, char *name, size_t cap) try { if (cu) *cu = 1; if (mhz) *mhz = 0; if (name && cap) snprintf(name, cap, "emulation"); return ZK_OK; } ZK_GUARD
#endif

static int fail(int code, const char *msg) { return fail_msg(code, msg); }
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static_assert(sizeof(G1::Affine) == 64 && sizeof(G2::Affine) == 128, "affine layouts must match the .raw / libff memory image");
static_assert(sizeof(G1::XYZZ) == 128 && sizeof(G2::XYZZ) == 256, "XYZZ layouts");
static_assert(sizeof(zk_partials) == 640, "zk_partials layout");

// ================================================================ library / device
extern "C" const char *zk_version(void) {
#ifdef ZK_EMUL
    return "zkhip 0.4.0 (CPU EMULATION BUILD - tests only)";
#else
    return "zkhip 0.4.0 (gfx950)";
#endif
}
extern "C" uint32_t zk_abi_version(void) { return ZK_ABI_VERSION; }
extern "C" const char *zk_strerror(int code) {
    switch (code) {
    case ZK_OK: return "ok";
    case ZK_ERR_ARG: return "invalid argument";
    case ZK_ERR_IO: return "file i/o error";
    case ZK_ERR_FORMAT: return "malformed proving key stream";
    case ZK_ERR_HIP: return "HIP runtime error";
    case ZK_ERR_NOMEM: return "out of memory";
    case ZK_ERR_SHAPE: return "proving key does not match the constraint system";
    case ZK_ERR_DEGREE: return "H polynomial has wrong degree (witness does not satisfy the R1CS)";
    case ZK_ERR_NODEVICE: return "no HIP device";
    case ZK_ERR_BUFFER: return "output buffer too small";
    case ZK_ERR_INTERNAL: return "internal error (exception caught at the C ABI)";
    default: return "unknown error";
    }
}
extern "C" const char *zk_last_error(void) { return g_last_error; }
extern "C" int zk_device_count(int *count) try {
    if (!count) return ZK_ERR_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(ZK_ERR_NODEVICE, "hipGetDeviceCount failed: no usable HIP device"); }
    *count = n;
    return ZK_OK;
} ZK_GUARD
// RAII: run a block on `device` and hand the caller's current device back (destructors and frees run from wherever the caller is)
namespace {
struct DeviceScope {
    int prev = -1; bool switched = false;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace
static int use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ZK_ERR_NODEVICE, "no HIP device (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(ZK_ERR_ARG, "device ordinal out of range");
    ZK_HIP(hipSetDevice(device));
    return ZK_OK;
}

// ================================================================ proving key (host)
static std::atomic<uint64_t> g_pk_ids{1};
struct zk_pk {
    const uint64_t id = g_pk_ids.fetch_add(1);          // identity of the key for the device-table cache below
    G1::Affine alpha_g1, beta_g1, delta_g1;
    G2::Affine beta_g2, delta_g2;
    uint32_t a_domain = 0, b_domain = 0;
    std::vector<uint32_t> a_idx, b_idx;
    std::vector<G1::Affine> a_val, H, L;
    std::vector<G2::Affine> b_val;
    // the G1 half of the B-query's knowledge commitments (full key stream, tcc:53-90): same length and indices as b_val.
    // A key with it (zk_pk_load_raw_full, zk_keygen_full) can make zero-knowledge proofs; a nozk key leaves it empty.
    bool full = false;
    std::vector<G1::Affine> b1_val;
};

extern "C" int zk_pk_from_parts(const uint64_t *alpha_g1, const uint64_t *beta_g1, const uint64_t *beta_g2,
                                const uint64_t *delta_g1, const uint64_t *delta_g2,
                                uint32_t a_domain, uint32_t nA, const uint32_t *a_idx, const uint64_t *a_val,
                                uint32_t b_domain, uint32_t nB, const uint32_t *b_idx, const uint64_t *b_val,
                                uint32_t nH, const uint64_t *H, uint32_t nL, const uint64_t *L, zk_pk **out) try {
    if (!alpha_g1 || !beta_g1 || !beta_g2 || !delta_g1 || !delta_g2 || !out) return fail(ZK_ERR_ARG, "null argument");
    if ((nA && (!a_idx || !a_val)) || (nB && (!b_idx || !b_val)) || (nH && !H) || (nL && !L)) return fail(ZK_ERR_ARG, "null query array");
    // sizes a domain of at most 2^28 (the 2-adicity of r - 1, src/stubs.cpp:49-75) can produce; anything larger is a caller error
    const uint64_t lim = (1ull << 28) + 1;
    if (a_domain > lim || b_domain > lim || nA > a_domain || nB > b_domain || nH > lim || nL > lim) return fail(ZK_ERR_ARG, "query sizes exceed their domain (or the 2^28 limit of the evaluation domain)");
    std::unique_ptr<zk_pk> pk(new zk_pk());
    // all host memory is claimed BEFORE the first byte of the caller's arrays is read: a size the host cannot hold ends in
    // ZK_ERR_NOMEM (ZK_GUARD), not in a half-copied key
    pk->a_idx.resize(nA); pk->b_idx.resize(nB); pk->a_val.resize(nA); pk->b_val.resize(nB); pk->H.resize(nH); pk->L.resize(nL);
    memcpy(&pk->alpha_g1, alpha_g1, 64); memcpy(&pk->beta_g1, beta_g1, 64); memcpy(&pk->beta_g2, beta_g2, 128);
    memcpy(&pk->delta_g1, delta_g1, 64); memcpy(&pk->delta_g2, delta_g2, 128);
    pk->a_domain = a_domain; pk->b_domain = b_domain;
    if (nA) { memcpy(pk->a_idx.data(), a_idx, 4 * (size_t)nA); memcpy(pk->a_val.data(), a_val, 64 * (size_t)nA); }
    if (nB) { memcpy(pk->b_idx.data(), b_idx, 4 * (size_t)nB); memcpy(pk->b_val.data(), b_val, 128 * (size_t)nB); }
    if (nH) memcpy(pk->H.data(), H, 64 * (size_t)nH);
    if (nL) memcpy(pk->L.data(), L, 64 * (size_t)nL);
    for (uint32_t k = 0; k < nA; k++) if (a_idx[k] >= a_domain || (k && a_idx[k] <= a_idx[k - 1])) return fail(ZK_ERR_ARG, "A_query indices must be ascending and inside the domain");
    for (uint32_t k = 0; k < nB; k++) if (b_idx[k] >= b_domain || (k && b_idx[k] <= b_idx[k - 1])) return fail(ZK_ERR_ARG, "B_query indices must be ascending and inside the domain");
    *out = pk.release();
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_pk_sizes(const zk_pk *pk, uint32_t s[6]) try {
    if (!pk || !s) return ZK_ERR_ARG;
    s[0] = pk->a_domain; s[1] = (uint32_t)pk->a_idx.size(); s[2] = pk->b_domain; s[3] = (uint32_t)pk->b_idx.size();
    s[4] = (uint32_t)pk->H.size(); s[5] = (uint32_t)pk->L.size();
    return ZK_OK;
} ZK_GUARD
extern "C" const void *zk_pk_part(const zk_pk *pk, int which) {
    if (!pk) return nullptr;
    switch (which) {
    case 0: return &pk->alpha_g1; case 1: return &pk->beta_g1; case 2: return &pk->beta_g2;
    case 3: return &pk->delta_g1; case 4: return &pk->delta_g2;
    case 5: return pk->a_idx.data(); case 6: return pk->a_val.data(); case 7: return pk->b_idx.data(); case 8: return pk->b_val.data();
    case 9: return pk->H.data(); case 10: return pk->L.data(); case 11: return pk->b1_val.data(); default: return nullptr;
    }
}
namespace { void tables_drop_key(uint64_t pk_id); }
extern "C" void zk_pk_free(zk_pk *pk) try { if (pk) tables_drop_key(pk->id); delete pk; } ZK_GUARD_VOID

// ---- .raw stream under BINARY_OUTPUT + MONTGOMERY_OUTPUT + NO_PT_COMPRESSION (CMakeLists.txt:115-131,186-188):
// point = ASCII '0'/'1' infinity flag + raw Montgomery limbs (G1: X Y; G2: X.c0 X.c1 Y.c0 Y.c1); infinity carries affine
// X = 0, Y = 1; vector = decimal size "\n" elements; sparse_vector = domain "\n" count "\n" indices (one per line)
// count "\n" elements; knowledge_commitment<G2, G1> = g then h.
//   ZK_CODEC_ALT_BN128: upstream libff alt_bn128_G1/G2 stream operators.
//   ZK_CODEC_MCL_BN128: the fork's default curve build (CMakeLists.txt:47-54).  Its mcl_bn128_G1/G2 stream operators are
//     in the ABSENT libff fork; inferred from upstream libff's bn128 (ate-pairing) wrapper they are modelled on: the same
//     flag + raw coordinate memory, and mcl keeps Fp in Montgomery form with R = 2^256 -- i.e. the SAME BYTES.
//     PARITY UNPINNED: the reference holds no key file; a verified layout would replace point()/put_point() below.
namespace {
bool codec_known(int codec) { return codec == ZK_CODEC_ALT_BN128 || codec == ZK_CODEC_MCL_BN128; }
struct RawReader {
    FILE *f; int codec; bool bad = false;
    uint64_t left = ~0ull;                  // bytes the stream can still hold (regular files: fstat size - position; pipes: unknown)
    static constexpr uint64_t CHUNK = 1u << 16;   // elements a vector grows by while it is being read: nothing is allocated for
                                                  // a count the stream has not yet proven it holds
    RawReader(FILE *f_, int codec_) : f(f_), codec(codec_) {
        struct stat st;
        if (f && fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode)) { const off_t at = ftello(f); left = at >= 0 && st.st_size >= at ? (uint64_t)(st.st_size - at) : 0; }
    }
    int get() { const int c = fgetc(f); if (c != EOF && left != ~0ull && left) left--; return c; }
    template <class P> void point(P &p) {
        int c = get();
        if (c != '0' && c != '1') { bad = true; return; }
        if (fread(&p, sizeof(P), 1, f) != 1) { bad = true; return; }
        if (left != ~0ull) left = left >= sizeof(P) ? left - sizeof(P) : 0;
        if (c == '1') memset(&p, 0, sizeof(P));
    }
    uint64_t size() {
        uint64_t v = 0; int c, nd = 0;
        while ((c = get()) >= '0' && c <= '9') { v = v * 10 + (uint64_t)(c - '0'); if (++nd > 12) { bad = true; return 0; } }
        if (c != '\n' || nd == 0) bad = true;
        return v;
    }
    // a declared element count is believed only as far as the rest of the stream can hold it (min_bytes per element)
    bool fits(uint64_t n, uint64_t min_bytes) {
        if (n > (1ull << 28) + 1) return false;
        return left == ~0ull || n <= left / min_bytes;
    }
    template <class P> void points(std::vector<P> &v, uint64_t n) {
        if (bad) return;
        if (!fits(n, 1 + sizeof(P))) { bad = true; return; }
        v.clear();
        for (uint64_t i = 0; i < n && !bad;) {
            const uint64_t upto = n - i < CHUNK ? n : i + CHUNK;
            v.resize(upto);
            for (; i < upto && !bad; i++) point(v[i]);
        }
    }
    // sparse_vector header: domain, indices; returns the value count
    uint64_t sparse_head(uint32_t &domain, std::vector<uint32_t> &idx) {
        if (bad) return 0;
        const uint64_t dom = size();
        if (dom > (1ull << 28) + 1) { bad = true; return 0; }
        domain = (uint32_t)dom;
        uint64_t n = size();
        if (bad || n > dom || !fits(n, 2)) { bad = true; return 0; }       // an index is at least one digit and a newline
        idx.clear();
        for (uint64_t i = 0; i < n && !bad;) {
            const uint64_t upto = n - i < CHUNK ? n : i + CHUNK;
            idx.resize(upto);
            for (; i < upto && !bad; i++) {
                const uint64_t x = size();
                idx[i] = (uint32_t)x;
                if (x >= domain || (i && idx[i] <= idx[i - 1])) bad = true;
            }
        }
        uint64_t nv = size();
        if (nv != n) bad = true;
        return bad ? 0 : nv;
    }
};
struct FileCloser { FILE *f; ~FileCloser() { if (f) fclose(f); } };
struct RawWriter {
    FILE *f; int codec;
    G1::Affine i1; G2::Affine i2;
    RawWriter(FILE *f_, int codec_) : f(f_), codec(codec_) { i1.x = Fq::zero(); i1.y = Fq::one(); i2.x = Fq2::zero(); i2.y = Fq2::one(); }
    void point(const G1::Affine &p) { const bool inf = G1::is_inf(p); fputc(inf ? '1' : '0', f); fwrite(inf ? &i1 : &p, sizeof(p), 1, f); }
    void point(const G2::Affine &p) { const bool inf = G2::is_inf(p); fputc(inf ? '1' : '0', f); fwrite(inf ? &i2 : &p, sizeof(p), 1, f); }
    template <class P> void points(const std::vector<P> &v) { fprintf(f, "%zu\n", v.size()); for (auto &p : v) point(p); }
    void sparse_head(uint32_t domain, const std::vector<uint32_t> &idx) {
        fprintf(f, "%u\n%zu\n", domain, idx.size());
        for (uint32_t i : idx) fprintf(f, "%u\n", i);
        fprintf(f, "%zu\n", idx.size());
    }
};
}  // namespace

extern "C" int zk_pk_load_raw(const char *path, int codec, zk_pk **out) try {
    if (!path || !out) return fail(ZK_ERR_ARG, "null argument");
    if (!codec_known(codec)) return fail(ZK_ERR_ARG, "unsupported codec (ZK_CODEC_ALT_BN128 or ZK_CODEC_MCL_BN128)");
    FileCloser fc{fopen(path, "rb")};
    FILE *f = fc.f;
    if (!f) return fail(ZK_ERR_IO, "cannot open proving key file");       // reference: assert(fh.is_open()), utils.hpp:180
    std::unique_ptr<zk_pk> pk(new zk_pk());                                 // (an exception on the way leaves nothing behind: ZK_GUARD)
    RawReader r(f, codec);
    r.point(pk->alpha_g1); r.point(pk->beta_g1); r.point(pk->beta_g2); r.point(pk->delta_g1); r.point(pk->delta_g2);
    r.points(pk->a_val, r.sparse_head(pk->a_domain, pk->a_idx));
    r.points(pk->b_val, r.sparse_head(pk->b_domain, pk->b_idx));
    if (!r.bad) r.points(pk->H, r.size());
    if (!r.bad) r.points(pk->L, r.size());
    if (r.bad) return fail(ZK_ERR_FORMAT, "malformed .raw proving key stream (bad token, or a count the file cannot hold)");
    *out = pk.release();
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_pk_save_raw(const zk_pk *pk, const char *path, int codec) try {
    if (!pk || !path) return fail(ZK_ERR_ARG, "null argument");
    if (!codec_known(codec)) return fail(ZK_ERR_ARG, "unsupported codec (ZK_CODEC_ALT_BN128 or ZK_CODEC_MCL_BN128)");
    FILE *f = fopen(path, "wb");
    if (!f) return fail(ZK_ERR_IO, "cannot create proving key file");
    RawWriter w(f, codec);
    w.point(pk->alpha_g1); w.point(pk->beta_g1); w.point(pk->beta_g2); w.point(pk->delta_g1); w.point(pk->delta_g2);
    w.sparse_head(pk->a_domain, pk->a_idx); for (auto &p : pk->a_val) w.point(p);
    w.sparse_head(pk->b_domain, pk->b_idx); for (auto &p : pk->b_val) w.point(p);
    w.points(pk->H); w.points(pk->L);
    bool bad = ferror(f) != 0;
    if (fclose(f) != 0) bad = true;
    return bad ? fail(ZK_ERR_IO, "write error") : ZK_OK;
} ZK_GUARD

// ---- the reference's offline key converters over the FULL (zero-knowledge) proving key stream, tcc:53-90:
// alpha_g1 beta_g1 beta_g2 delta_g1 delta_g2, A_query (vector<G1>, V + 1 entries, zeros included), B_query
// (knowledge_commitment_vector<G2, G1>: sparse, each value = G2 then G1), H_query, L_query.
namespace {
struct FullKey {
    G1::Affine alpha_g1, beta_g1, delta_g1; G2::Affine beta_g2, delta_g2;
    std::vector<G1::Affine> A, Bh, H, L;
    uint32_t b_domain = 0; std::vector<uint32_t> b_idx; std::vector<G2::Affine> Bg;
};
int full_load(const char *path, int codec, FullKey &k) {
    FileCloser fc{fopen(path, "rb")};
    FILE *f = fc.f;
    if (!f) return fail(ZK_ERR_IO, "cannot open proving key file");
    RawReader r(f, codec);
    r.point(k.alpha_g1); r.point(k.beta_g1); r.point(k.beta_g2); r.point(k.delta_g1); r.point(k.delta_g2);
    if (!r.bad) r.points(k.A, r.size());
    const uint64_t nb = r.sparse_head(k.b_domain, k.b_idx);
    if (!r.bad && !r.fits(nb, 2 + sizeof(G2::Affine) + sizeof(G1::Affine))) r.bad = true;
    for (uint64_t i = 0; i < nb && !r.bad; i++) {
        if (i % RawReader::CHUNK == 0) { const uint64_t upto = nb - i < RawReader::CHUNK ? nb : i + RawReader::CHUNK; k.Bg.resize(upto); k.Bh.resize(upto); }
        r.point(k.Bg[i]); r.point(k.Bh[i]);
    }
    if (!r.bad) r.points(k.H, r.size());
    if (!r.bad) r.points(k.L, r.size());
    return r.bad ? fail(ZK_ERR_FORMAT, "malformed proving key stream") : ZK_OK;
}
int full_save(const char *path, int codec, const FullKey &k) {
    FILE *f = fopen(path, "wb");
    if (!f) return fail(ZK_ERR_IO, "cannot create proving key file");
    RawWriter w(f, codec);
    w.point(k.alpha_g1); w.point(k.beta_g1); w.point(k.beta_g2); w.point(k.delta_g1); w.point(k.delta_g2);
    w.points(k.A);
    w.sparse_head(k.b_domain, k.b_idx);
    for (size_t i = 0; i < k.Bg.size(); i++) { w.point(k.Bg[i]); w.point(k.Bh[i]); }
    w.points(k.H); w.points(k.L);
    bool bad = ferror(f) != 0;
    if (fclose(f) != 0) bad = true;
    return bad ? fail(ZK_ERR_IO, "write error") : ZK_OK;
}
// G1T_alt2mcl / G2T_alt2mcl (export.cpp:330-350): every coordinate travels as the DECIMAL string of its canonical value
// (bigintToString(X.as_bigint())) and is parsed again on the other side; Z is 1, or the point is (0, 1, 0)
std::string fq_to_decimal(const fe &mont) {
    fe c = Fq::from_mont(mont);
    uint32_t l[8]; for (int i = 0; i < 8; i++) l[i] = c.l[i];
    std::string out;
    for (;;) {
        uint64_t rem = 0; bool any = false;
        for (int i = 7; i >= 0; i--) { uint64_t cur = (rem << 32) | l[i]; l[i] = (uint32_t)(cur / 1000000000u); rem = cur % 1000000000u; any |= l[i] != 0; }
        char buf[16]; snprintf(buf, sizeof(buf), any ? "%09u" : "%u", (unsigned)rem);
        out.insert(0, buf);
        if (!any) break;
    }
    return out;
}
bool fq_from_decimal_str(const std::string &s, fe &out) {
    fe acc = Fq::zero(); const fe ten = Fq::from_u64(10);
    if (s.empty()) return false;
    for (char ch : s) { if (ch < '0' || ch > '9') return false; acc = Fq::add(Fq::mul(acc, ten), Fq::from_u64((uint64_t)(ch - '0'))); }
    out = acc; return true;
}
bool through_decimal(fe &v) { return fq_from_decimal_str(fq_to_decimal(v), v); }
bool through_decimal(G1::Affine &p) { return G1::is_inf(p) || (through_decimal(p.x) && through_decimal(p.y)); }
bool through_decimal(G2::Affine &p) { return G2::is_inf(p) || (through_decimal(p.x.c0) && through_decimal(p.x.c1) && through_decimal(p.y.c0) && through_decimal(p.y.c1)); }
}  // namespace

// pk_alt2mcl (src/export.cpp:352-397)
extern "C" int zk_pk_alt2mcl(const char *alt_pk_file, const char *mcl_pk_file) try {
    if (!alt_pk_file || !mcl_pk_file) return fail(ZK_ERR_ARG, "null argument");
    FullKey k;
    ZK_TRY(full_load(alt_pk_file, ZK_CODEC_ALT_BN128, k));
    bool ok = through_decimal(k.alpha_g1) && through_decimal(k.beta_g1) && through_decimal(k.beta_g2) && through_decimal(k.delta_g1) && through_decimal(k.delta_g2);
    for (auto &p : k.A) ok = ok && through_decimal(p);
    for (auto &p : k.Bg) ok = ok && through_decimal(p);
    for (auto &p : k.Bh) ok = ok && through_decimal(p);
    for (auto &p : k.H) ok = ok && through_decimal(p);
    for (auto &p : k.L) ok = ok && through_decimal(p);
    if (!ok) return fail(ZK_ERR_FORMAT, "coordinate did not survive the decimal round trip");
    return full_save(mcl_pk_file, ZK_CODEC_MCL_BN128, k);
} ZK_GUARD

// pk_mcl2nozk (src/export.cpp:399-408) = loadFromFile<full key> + the nozk conversion of hpp:209-233
// the nozk conversion of hpp:209-233: the A-query keeps its non-zero entries, the B-query its G2 half
static void nozk_from_full(const FullKey &k, zk_pk &pk) {
    pk.alpha_g1 = k.alpha_g1; pk.beta_g1 = k.beta_g1; pk.beta_g2 = k.beta_g2; pk.delta_g1 = k.delta_g1; pk.delta_g2 = k.delta_g2;
    pk.a_domain = (uint32_t)k.A.size();
    for (size_t i = 0; i < k.A.size(); i++) if (!G1::is_inf(k.A[i])) { pk.a_idx.push_back((uint32_t)i); pk.a_val.push_back(k.A[i]); }
    pk.b_domain = k.b_domain; pk.b_idx = k.b_idx; pk.b_val = k.Bg;
    pk.H = k.H; pk.L = k.L;
}
extern "C" int zk_pk_mcl2nozk(const char *mcl_pk_file, const char *nozk_pk_file) try {
    if (!mcl_pk_file || !nozk_pk_file) return fail(ZK_ERR_ARG, "null argument");
    FullKey k;
    ZK_TRY(full_load(mcl_pk_file, ZK_CODEC_MCL_BN128, k));
    zk_pk pk;
    nozk_from_full(k, pk);
    return zk_pk_save_raw(&pk, nozk_pk_file, ZK_CODEC_MCL_BN128);
} ZK_GUARD

// ---- the full (zero-knowledge) key as a proving key: the nozk key zk_pk_mcl2nozk would make, plus the G1 half of the B-query
extern "C" int zk_pk_load_raw_full(const char *path, int codec, zk_pk **out) try {
    if (!path || !out) return fail(ZK_ERR_ARG, "null argument");
    if (!codec_known(codec)) return fail(ZK_ERR_ARG, "unsupported codec (ZK_CODEC_ALT_BN128 or ZK_CODEC_MCL_BN128)");
    FullKey k;
    ZK_TRY(full_load(path, codec, k));
    std::unique_ptr<zk_pk> pk(new zk_pk());
    nozk_from_full(k, *pk);
    pk->b1_val = std::move(k.Bh);
    pk->full = true;
    *out = pk.release();
    return ZK_OK;
} ZK_GUARD
// the full stream again: the A-query re-densified over a_domain (absent entries are the point at infinity)
extern "C" int zk_pk_save_raw_full(const zk_pk *pk, const char *path, int codec) try {
    if (!pk || !path) return fail(ZK_ERR_ARG, "null argument");
    if (!codec_known(codec)) return fail(ZK_ERR_ARG, "unsupported codec (ZK_CODEC_ALT_BN128 or ZK_CODEC_MCL_BN128)");
    if (!pk->full) return fail(ZK_ERR_ARG, "zk_pk_save_raw_full: the key has no G1 half of the B-query (a nozk key; load it with zk_pk_load_raw_full or make it with zk_keygen_full)");
    FullKey k;
    k.alpha_g1 = pk->alpha_g1; k.beta_g1 = pk->beta_g1; k.beta_g2 = pk->beta_g2; k.delta_g1 = pk->delta_g1; k.delta_g2 = pk->delta_g2;
    k.A.assign(pk->a_domain, G1::aff_infinity());
    for (size_t i = 0; i < pk->a_idx.size(); i++) k.A[pk->a_idx[i]] = pk->a_val[i];
    k.b_domain = pk->b_domain; k.b_idx = pk->b_idx; k.Bg = pk->b_val; k.Bh = pk->b1_val;
    k.H = pk->H; k.L = pk->L;
    return full_save(path, codec, k);
} ZK_GUARD
extern "C" int zk_pk_is_full(const zk_pk *pk) try { return pk && pk->full ? 1 : 0; } ZK_GUARD

// ================================================================ context
namespace {
struct DevCsr {
    uint32_t n_rows = 0, nnz = 0, n_long = 0, n_chunks = 0;
    uint32_t *row_ptr = nullptr, *col = nullptr, *long_row = nullptr, *long_first = nullptr, *chunk_begin = nullptr, *chunk_end = nullptr;
    fe *coeff = nullptr, *partial = nullptr;
    void release() {
        void *p[] = {row_ptr, col, long_row, long_first, chunk_begin, chunk_end, coeff, partial};
        for (void *q : p) if (q) hipFree(q);
        *this = DevCsr();
    }
    int upload(const zk_csr *m, uint32_t V, uint32_t batch) {
        n_rows = m->n_rows;
        nnz = m->row_ptr[n_rows];
        std::vector<uint32_t> lrow, lfirst, cb, ce;
        for (uint32_t j = 0; j < n_rows; j++) {
            uint32_t b = m->row_ptr[j], e = m->row_ptr[j + 1];
            if (e < b || e > nnz) return fail(ZK_ERR_ARG, "CSR row_ptr not monotone");
            if (e - b > SPMV_LONG_ROW) {
                lrow.push_back(j); lfirst.push_back((uint32_t)cb.size());
                for (uint32_t k = b; k < e; k += SPMV_CHUNK) { cb.push_back(k); ce.push_back(k + SPMV_CHUNK < e ? k + SPMV_CHUNK : e); }
            }
        }
        lfirst.push_back((uint32_t)cb.size());
        for (uint32_t k = 0; k < nnz; k++) if (m->col[k] > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables");
        n_long = (uint32_t)lrow.size(); n_chunks = (uint32_t)cb.size();
        ZK_HIP(hipMalloc(&row_ptr, 4 * (size_t)(n_rows + 1)));
        ZK_HIP(hipMalloc(&col, 4 * (size_t)(nnz + 1)));
        ZK_HIP(hipMalloc(&coeff, 32 * (size_t)(nnz + 1)));
        ZK_HIP(hipMemcpy(row_ptr, m->row_ptr, 4 * (size_t)(n_rows + 1), hipMemcpyHostToDevice));
        if (nnz) {
            ZK_HIP(hipMemcpy(col, m->col, 4 * (size_t)nnz, hipMemcpyHostToDevice));
            ZK_HIP(hipMemcpy(coeff, m->coeff, 32 * (size_t)nnz, hipMemcpyHostToDevice));
        }
        ZK_HIP(hipMalloc(&long_row, 4 * (size_t)(n_long + 1)));
        ZK_HIP(hipMalloc(&long_first, 4 * (size_t)(n_long + 1)));
        ZK_HIP(hipMalloc(&chunk_begin, 4 * (size_t)(n_chunks + 1)));
        ZK_HIP(hipMalloc(&chunk_end, 4 * (size_t)(n_chunks + 1)));
        ZK_HIP(hipMalloc(&partial, 32 * ((size_t)n_chunks * batch + 1)));
        if (n_long) ZK_HIP(hipMemcpy(long_row, lrow.data(), 4 * (size_t)n_long, hipMemcpyHostToDevice));
        ZK_HIP(hipMemcpy(long_first, lfirst.data(), 4 * (size_t)(n_long + 1), hipMemcpyHostToDevice));
        if (n_chunks) {
            ZK_HIP(hipMemcpy(chunk_begin, cb.data(), 4 * (size_t)n_chunks, hipMemcpyHostToDevice));
            ZK_HIP(hipMemcpy(chunk_end, ce.data(), 4 * (size_t)n_chunks, hipMemcpyHostToDevice));
        }
        return ZK_OK;
    }
    // out[p][0..n_rows) = M * w[p] for the `batch` witnesses w_stride elements apart (outputs out_stride apart)
    // m_rows >= n_rows: rows [n_rows, m_rows) of `out` are written too: the first n_in_rows of them w[0 ..), the rest zero (the polynomial's padding)
    int enqueue(const fe *w, fe *out, hipStream_t st, uint32_t batch, uint32_t w_stride, uint32_t out_stride, uint32_t m_rows = 0, uint32_t n_in_rows = 0) const {
        if (m_rows < n_rows) m_rows = n_rows;
        if (m_rows) ZK_LAUNCH(k_spmv_rows, dim3(zk_div_up(m_rows, 256), batch), 256, st, (const uint32_t *)row_ptr, (const uint32_t *)col, (const fe *)coeff, w, out, n_rows, w_stride, out_stride, m_rows, n_in_rows);
        if (n_chunks) {
            ZK_LAUNCH_SYNC(k_spmv_long_chunks, dim3(n_chunks, batch), 256, st, (const uint32_t *)chunk_begin, (const uint32_t *)chunk_end,
                           (const uint32_t *)col, (const fe *)coeff, w, partial, w_stride);
            ZK_LAUNCH_SYNC(k_spmv_long_finish, dim3(n_long, batch), 256, st, (const uint32_t *)long_row, (const uint32_t *)long_first,
                      (const fe *)partial, out, n_long, n_chunks, out_stride);
        }
        ZK_HIP(hipGetLastError());
        return ZK_OK;
    }
};

__global__ void k_to_mont(fe *a, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = Fr::to_mont(a[i]);
}
__global__ void k_field_mul(const fe *a, const fe *b, fe *o, uint32_t n, int field) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = field ? Fq::mul(a[i], b[i]) : Fr::mul(a[i], b[i]);
}

template <class T> int dev_upload(T **dst, const T *src, size_t n) {
    ZK_HIP(hipMalloc(dst, sizeof(T) * (n ? n : 1)));
    if (n) ZK_HIP(hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return ZK_OK;
}
struct Range { uint32_t lo, hi; uint32_t n() const { return hi - lo; } };
uint64_t csr_hash(const zk_csr *m, uint32_t a, uint32_t b, uint32_t c) {          // FNV-style hash over the words of the matrix and the circuit's shape
    uint64_t h = 1469598103934665603ull;
    auto eat = [&](const void *p, size_t n) {            // n: a multiple of 4; one multiplication per 32-bit word
        const uint32_t *q = (const uint32_t *)p;
        for (size_t i = 0; i < n / 4; i++) { h ^= q[i]; h *= 1099511628211ull; h ^= h >> 29; }
    };
    const uint32_t shape[4] = {m->n_rows, a, b, c};
    eat(shape, sizeof(shape));
    const uint32_t nnz = m->row_ptr[m->n_rows];
    eat(m->row_ptr, 4 * (size_t)(m->n_rows + 1)); eat(m->col, 4 * (size_t)nnz); eat(m->coeff, 32 * (size_t)nnz);
    return h;
}
Range shard_range(uint32_t n, uint32_t rank, uint32_t count) {
    return Range{(uint32_t)((uint64_t)n * rank / count), (uint32_t)((uint64_t)n * (rank + 1) / count)};
}
}  // namespace


// ---- window-multiple tables of one key shard on one device, shared by every context created for it
// (the reference shares one ProvingKeyT among ProverContexts the same way, hpp:279-291): 5 GB at n = 2^20.
namespace {
struct DeviceTables {
    uint64_t pk_id = 0; int device = 0; uint32_t rank = 0, count = 1, cbits = 0;
    uint32_t max_batch = 1;                            // the window choice depends on the batch the contexts are built for (MsmShape::pick_c)
    uint32_t cA = 0, cB = 0, cH = 0, cL = 0;           // resolved window bits of the four tables
    G1::Affine *tA = nullptr, *tH = nullptr, *tL = nullptr; G2::Affine *tB = nullptr;
    uint32_t *dA_idx = nullptr, *dB_idx = nullptr;
    // zero-knowledge proofs (a full key, unsharded): the G1 half of the B-query tabulated with the B-query's window bits and
    // rows -- its multi-exponentiation reads the B-query's sorted entries --, and the fixed-base tables of delta1 / delta2 (blind.hpp)
    bool zk = false;
    G1::Affine *tB1 = nullptr, *tD1 = nullptr; G2::Affine *tD2 = nullptr;
    // the A-, B- and L-query all read the witness: ONE bucket sort of all V+1 witness digits drives every query that
    // holds at least 7/8 of the variables (absent entries are skipped lane-locally); sparser queries and sharded
    // contexts sort their own scalars
    bool share_A = false, share_B = false, share_L = false;
    uint32_t win_lo = 0, win_n = 0;                    // the witness window [win_lo, win_lo + win_n) the shared sort covers: all V + 1 variables
                                                       // when unsharded, the span of this shard's A / B / L entries otherwise
    uint32_t *posA = nullptr, *posB = nullptr;         // window position -> entry of this shard's query (0xffffffff: none); nullptr: position - offX
    uint32_t offA = 0, offB = 0, offL = 0;
    uint32_t cW = 0;                                   // window bits of the shared witness sort and of the tables it drives
    uint32_t plog = 0;                                 // memory-frugal tables: every 2^plog-th window only (MsmShape::plog); 0 = all W windows
    uint64_t table_bytes = 0, full_table_bytes = 0;    // what the four tables take, and what they would take with every window
    // the H-query in coset-Lagrange bases (hlagrange.hpp): tH holds the m bases Q_j and tL the V + 1 bases L_v - K_v instead of
    // the key's H- and L-query.  They depend on the circuit's C matrix as well as on the key: `circ` (a hash of it) is part of what a context
    // looks its tables up by.  lag_req: what the contexts of this set asked for (a set whose tables came out frugal proves in the key's bases)
    bool lag_req = false, lag = false;
    uint64_t circ = 0;
    double lag_ms = 0;                                 // what the transform of the bases took, once (zk_ctx_hlagrange_info)
    bool key_alive = true;                             // false once zk_pk_free has run: the last context to go takes the tables along
    int refs = 0;
    // device memory of the set; leaves the caller's current device as it found it (zk_pk_free runs this from wherever the
    // caller is -- Python's garbage collector inside a torch process -- and an eviction runs it in the middle of ctx_build)
    void free_device() {
        DeviceScope on(device);
        void *dev[] = {tA, tH, tL, tB, dA_idx, dB_idx, posA, posB, tB1, tD1, tD2};
        for (void *p : dev) if (p) hipFree(p);
        tA = tH = tL = nullptr; tB = nullptr; dA_idx = dB_idx = posA = posB = nullptr; tB1 = tD1 = nullptr; tD2 = nullptr;
    }
};
struct DeviceTablesDeleter { void operator()(DeviceTables *t) const { if (t) { t->free_device(); delete t; } } };
std::mutex g_tables_mu;
std::vector<DeviceTables *> g_tables;

template <class C>
int build_table(typename C::Affine **out, const typename C::Affine *host_bases, uint32_t n, uint32_t cbits, uint32_t plog = 0) {
    MsmWork<C> tmp;                                      // only to own the expansion; its scratch is released again
    typename C::Affine *d_bases = nullptr;
    tmp.sh.set(n ? n : 1, cbits, 1, plog);
    tmp.table_n = n;
    int rc = ZK_OK;
    if (hipMalloc(&tmp.table, sizeof(typename C::Affine) * (size_t)(n ? n : 1) * tmp.sh.rows()) != hipSuccess) { (void)hipGetLastError(); rc = fail_msg(ZK_ERR_NOMEM, "out of device memory for the window-multiple tables"); }
    if (rc == ZK_OK) rc = dev_upload(&d_bases, host_bases, n);
    if (rc == ZK_OK) rc = tmp.precompute(d_bases, n, nullptr);
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "k_msm_precompute failed");
    if (d_bases) hipFree(d_bases);
    if (rc == ZK_OK) { *out = tmp.table; tmp.owns_table = false; }      // keep the table, drop the rest
    tmp.release();
    return rc;
}
// the same expansion of bases that already lie in device memory
template <class C>
int build_table_dev(typename C::Affine **out, const typename C::Affine *d_bases, uint32_t n, uint32_t cbits, uint32_t plog = 0) {
    MsmWork<C> tmp;
    tmp.sh.set(n ? n : 1, cbits, 1, plog);
    tmp.table_n = n;
    int rc = ZK_OK;
    if (hipMalloc(&tmp.table, sizeof(typename C::Affine) * (size_t)(n ? n : 1) * tmp.sh.rows()) != hipSuccess) { (void)hipGetLastError(); rc = fail_msg(ZK_ERR_NOMEM, "out of device memory for the window-multiple tables"); }
    if (rc == ZK_OK) rc = tmp.precompute(d_bases, n, nullptr);
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "k_msm_precompute failed");
    if (rc == ZK_OK) { *out = tmp.table; tmp.owns_table = false; }
    tmp.release();
    return rc;
}
struct DevScratch {                                     // device buffers of one construction step, released with it
    std::vector<void *> p;
    template <class T> int get(T **out, size_t n) { ZK_HIP(hipMalloc(out, sizeof(T) * (n ? n : 1))); p.push_back(*out); return ZK_OK; }
    template <class T> int put(T **out, const T *src, size_t n) { ZK_TRY(get(out, n)); if (n) ZK_HIP(hipMemcpy(*out, src, sizeof(T) * n, hipMemcpyHostToDevice)); return ZK_OK; }
    ~DevScratch() { for (void *q : p) hipFree(q); }
};
// The bases of the four-transform prover (hlagrange.hpp): d_q[0 .. m) = Q_j and d_lk[0 .. V] = L_v - K_v, affine, in device memory
// of the caller.  H: the key's m - 1 H-query bases, L: its V - nIn L-query bases (host), Cm: the circuit's C matrix.
// d_lk[v] = L_v - K_v for v <= V, K_v = sum_j C[j][v] Lambda_j: d_lam the m bases Lambda_j (device), L the V - nIn L-query bases (host)
int hl_column_bases(const G1::Affine *d_lam, const G1::Affine *L, const zk_csr *Cm, uint32_t nIn, uint32_t V, G1::Affine *d_lk) {
    DevScratch s;
    G1::Affine *d_l = nullptr; G1::XYZZ *d_part = nullptr;
    // C by columns, every column cut into chunks of HL_COL_CHUNK entries
    const uint32_t nnz = Cm->row_ptr[Cm->n_rows];
    std::vector<uint32_t> cnt(V + 2, 0), row(nnz ? nnz : 1), cb, ce, first(V + 2, 0);
    std::vector<fe> cf(nnz ? nnz : 1);
    for (uint32_t k = 0; k < nnz; k++) { if (Cm->col[k] > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables"); cnt[Cm->col[k] + 1]++; }
    for (uint32_t v = 0; v <= V; v++) cnt[v + 1] += cnt[v];
    {
        std::vector<uint32_t> at(cnt.begin(), cnt.end() - 1);
        for (uint32_t j = 0; j < Cm->n_rows; j++)
            for (uint32_t k = Cm->row_ptr[j]; k < Cm->row_ptr[j + 1]; k++) { const uint32_t o = at[Cm->col[k]]++; row[o] = j; memcpy(&cf[o], Cm->coeff + 4 * (size_t)k, 32); }
    }
    for (uint32_t v = 0; v <= V; v++) {
        first[v] = (uint32_t)cb.size();
        for (uint32_t k = cnt[v]; k < cnt[v + 1]; k += HL_COL_CHUNK) { cb.push_back(k); ce.push_back(k + HL_COL_CHUNK < cnt[v + 1] ? k + HL_COL_CHUNK : cnt[v + 1]); }
    }
    first[V + 1] = (uint32_t)cb.size();
    const uint32_t n_chunks = (uint32_t)cb.size();
    uint32_t *d_row = nullptr, *d_cb = nullptr, *d_ce = nullptr, *d_first = nullptr; fe *d_cf = nullptr;
    ZK_TRY(s.put(&d_row, row.data(), nnz)); ZK_TRY(s.put(&d_cf, cf.data(), nnz));
    ZK_TRY(s.put(&d_cb, cb.data(), n_chunks)); ZK_TRY(s.put(&d_ce, ce.data(), n_chunks)); ZK_TRY(s.put(&d_first, first.data(), first.size()));
    ZK_TRY(s.put(&d_l, L, V - nIn));
    ZK_TRY(s.get(&d_part, n_chunks));
    if (n_chunks) ZK_LAUNCH(k_hl_col_chunks, zk_div_up(n_chunks, 64), 64, nullptr, (const uint32_t *)d_cb, (const uint32_t *)d_ce, n_chunks, (const uint32_t *)d_row,
                            (const fe *)d_cf, (const G1::Affine *)d_lam, d_part);
    ZK_LAUNCH(k_hl_col_finish, zk_div_up(V + 1, 64), 64, nullptr, (const uint32_t *)d_first, (const G1::XYZZ *)d_part, (const G1::Affine *)d_l, nIn + 1, V + 1, d_lk);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    return ZK_OK;
}
// d_out[0 .. m) = Lambda_j (coset = false) or Q_j (coset = true) of the n_in <= m points H (host)
int hl_group_dft(const G1::Affine *H, uint32_t n_in, uint32_t logm, bool coset, G1::Affine *d_out) {
    const uint32_t m = 1u << logm;
    DevScratch s;
    NttTables tab;
    struct TabFree { NttTables &t; ~TabFree() { ntt_tables_free(t); } } tab_free{tab};
    ZK_TRY(ntt_tables_create(tab, logm, nullptr));
    G1::Affine *d_h = nullptr; G1::XYZZ *d_work = nullptr;
    ZK_TRY(s.put(&d_h, H, n_in));
    ZK_TRY(s.get(&d_work, m));
    ZK_TRY(gdft_run(tab, d_h, n_in, coset, d_work, d_out, nullptr));
    ZK_HIP(hipDeviceSynchronize());
    return ZK_OK;
}
int hl_transform_bases(const G1::Affine *H, const G1::Affine *L, const zk_csr *Cm, uint32_t logm, uint32_t nIn, uint32_t V,
                       G1::Affine *d_q, G1::Affine *d_lk) {
    const uint32_t m = 1u << logm;
    DevScratch s;
    G1::Affine *d_lam = nullptr;
    ZK_TRY(s.get(&d_lam, m));
    ZK_TRY(hl_group_dft(H, m - 1, logm, true, d_q));
    ZK_TRY(hl_group_dft(H, m - 1, logm, false, d_lam));
    return hl_column_bases(d_lam, L, Cm, nIn, V, d_lk);
}
void tables_free_locked(DeviceTables *t);
// The tables belong to the KEY, not to the contexts that use them: the last context of a key leaves them in place (its next context -- the
// next leg of a benchmark, the next request -- finds them instead of expanding 5-20 GB again) and zk_pk_free drops them.
void tables_release(DeviceTables *t) {
    if (!t) return;
    std::lock_guard<std::mutex> lk(g_tables_mu);
    if (--t->refs <= 0 && !t->key_alive) tables_free_locked(t);
}
void tables_drop_key(uint64_t pk_id) {                  // zk_pk_free: every idle table set of the key, on every device
    std::lock_guard<std::mutex> lk(g_tables_mu);
    for (size_t i = 0; i < g_tables.size();) {
        DeviceTables *t = g_tables[i];
        if (t->pk_id == pk_id && t->refs <= 0) tables_free_locked(t);
        else { if (t->pk_id == pk_id) t->key_alive = false; i++; }
    }
}
// make room ON ONE DEVICE: drop an idle table set that lives there (least recently created first) -- of another key, or of this
// key in another shape (shard, window, batch: a set the context being built cannot use); true if something was freed.
// Sets on other devices are never touched: freeing them gives the device that is short of memory nothing.
bool tables_evict_idle_locked(int device) {
    for (size_t i = 0; i < g_tables.size(); i++)
        if (g_tables[i]->refs <= 0 && g_tables[i]->device == device) { tables_free_locked(g_tables[i]); return true; }
    return false;
}
void tables_free_locked(DeviceTables *t) {
    t->free_device();
    for (size_t i = 0; i < g_tables.size(); i++) if (g_tables[i] == t) { g_tables.erase(g_tables.begin() + i); break; }
    delete t;
}
}  // namespace

// ---- streams outlive the contexts that use them.  The runtime maps every stream to one of a few hardware queues when the
// stream is created and tears the queue down with its last stream; a context set created after an earlier one was destroyed
// got another mapping and proved 6 % slower at 2^20 (9.4 -> 10.0 ms per proof, same kernels: tools/dev_second_leg.py).  A closed
// context therefore parks its streams here, by device, role and priority, and the next context of that role takes them in the
// order they were parked: the n-th context of a process always runs on the same queues.  Parked streams are idle (the
// destructor drains them) and are released with the process.
namespace {
struct ParkedStream { int device, role, prio; hipStream_t st; };
std::mutex g_streams_mu;
std::vector<ParkedStream> g_streams;
int stream_take(hipStream_t *out, int device, int role, int prio) {
    {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        for (size_t i = 0; i < g_streams.size(); i++)
            if (g_streams[i].device == device && g_streams[i].role == role && g_streams[i].prio == prio) {
                *out = g_streams[i].st; g_streams.erase(g_streams.begin() + i); return ZK_OK;
            }
    }
    ZK_HIP(hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio));
    return ZK_OK;
}
void stream_park(hipStream_t st, int device, int role, int prio) {
    if (!st) return;
    (void)hipStreamSynchronize(st);
    std::lock_guard<std::mutex> lk(g_streams_mu);
    g_streams.push_back(ParkedStream{device, role, prio, st});
}
enum { ROLE_MAIN = 0, ROLE_ACC, ROLE_A, ROLE_B, ROLE_L, ROLE_COPY };
}  // namespace

// proofs in flight per device, over all contexts of the process: a proof that is queued while nothing else is in flight will (start to) run
// alone on the machine, whichever entry point it came through, and takes the latency shapes of the bucket reductions (four lanes per point
// operation, the whole workgroup per row: zk_prove's); proofs queued behind others are throughput work
namespace { std::atomic<int> g_dev_inflight[64]; }
struct zk_ctx {
    int device = 0;
    int stream_prio[6] = {0, 0, 0, 0, 0, 0};   // priority each role's stream was taken with (stream_park files it under the same key)
    DeviceTables *tables = nullptr;
    bool serial = false;
    bool in_flight = false;
    bool alone_hint = false;                   // nothing else was in flight on this device when the proof was queued
    void set_in_flight(bool on) {
        if (on != in_flight && device >= 0 && device < 64) g_dev_inflight[device].fetch_add(on ? 1 : -1, std::memory_order_relaxed);
        in_flight = on;
    }
    bool awaiting_h = false;                   // the proof in flight was submitted without its H part (zk_prove_submit_defer_h): zk_prove_submit_h completes it
    uint32_t max_batch = 1, cur_batch = 1;     // proofs per launch sequence: capacity, and of the proof(s) in flight
    uint32_t nC = 0, nIn = 0, V = 0, m = 0, logm = 0;
    zk_config cfg{};
    G1::Affine alpha_g1; G2::Affine beta_g2;
    // shard-local base ranges (whole query when unsharded)
    Range rA{}, rB{}, rH{}, rL{};
    uint32_t *dA_idx = nullptr, *dB_idx = nullptr;
    DevCsr cA, cB, cC;
    fe *d_w = nullptr, *d_a = nullptr, *d_b = nullptr, *d_c = nullptr, *d_t = nullptr;
    uint8_t *d_partials = nullptr;             // 640 bytes: the four partial sums in zk_partials layout, device copy
    fe *h_w = nullptr;                         // pinned staging for the witness
    // double-buffered upload (zk_prove_stage): second device / pinned buffer pair, copy stream, allocated on first use
    fe *d_w2 = nullptr, *h_w2 = nullptr;
    hipStream_t s_copy = nullptr;
    hipEvent_t ev_staged = nullptr;
    uint32_t staged_k = 0; int staged_canonical = 0;
    fe *h_tail = nullptr;                      // pinned: h[m-1] for the degree check
    NttTables tab;
    MsmWork<G1> mA, mH, mL, mW; MsmWork<G2> mB;       // mW: sort-only, the shared witness-digit sort
    // zero-knowledge proofs (a context of a full key, tables->zk): the G1 half of the B-query (driven by the B-query's sort) and the
    // blinding buffers (blind.hpp), device and pinned host copy: [k x {r, s}][k x {A, C}][k x B] for k = max_batch, on the device followed by
    // [k x {r delta1, s delta1, -rs delta1}].  cur_zk: the proof in flight is one.  ev_z1 / ev_z2: after k_zk_blind_g1 / _g2 (zk_timings.gpu_total)
    MsmWork<G1> mB1;
    uint8_t *d_zk = nullptr, *h_zk = nullptr;
    G1::Affine beta_g1;
    bool cur_zk = false;
    hipEvent_t ev_z1 = nullptr, ev_z2 = nullptr, ev_zf = nullptr;          // ev_zf: after k_zk_blind_fixed
    hipStream_t s_main = nullptr, s_acc = nullptr, s_a = nullptr, s_b = nullptr, s_l = nullptr;
    hipStream_t s_h = nullptr;                 // the H pipeline (row evaluations, transforms, H sort and tail) beside the witness sorts; == s_main when not split
    hipEvent_t ev_up = nullptr, ev_sort_h = nullptr;
    bool h_stream_made = false;
    bool latency_call = false;                 // the proof being queued came through a synchronous entry point (zk_prove ...)
    // C = Ht + Lt is the only use of the H- and L-query results (tcc:540): when both multi-exponentiations have the same bucket set
    // (same window bits) the L-query's chunk pieces are folded into the H-query's bucket reduction -- one tail (finalize, heavy, group
    // reduce, tree sums) per proof less; zk_partials then carries the sum in Ht and the point at infinity in Lt.  ZK_NO_MERGE_HL=1: off.
    bool merge_hl = false;
    // the four-transform prover (hlagrange.hpp): this context's tables hold the H-query in coset-Lagrange bases and the L-query over all V + 1
    // variables.  l_first: the first variable of the L-query (0, or nIn + 1 in the key's bases).  d_bscale: g^i / (m R), the post-scale of B's inverse
    // transform; d_hpart: the workgroups' shares of the degree check's two sums; d_tail: h[m-1] per proof; kp, kc, zg: constants of k_hl_tail / k_hl_q_from_h
    bool lag = false;
    uint32_t l_first = 0;
    fe *d_bscale = nullptr, *d_hpart = nullptr, *d_tail = nullptr;
    fe hl_kp, hl_kc, hl_zg;
    bool cur_merge = false;                    // ... and whether the proof in flight does it (a small synchronous proof keeps two tails: see prove_enqueue)
    // tuning aids, read from the environment ONCE at context creation (never on the proving path)
    bool env_no_direct_h2d = false;            // ZK_NO_DIRECT_H2D: synchronous proofs stage the witness through pinned memory too
    int env_h_stream = -1;                     // ZK_H_STREAM=0 / 1 forces the H pipeline onto s_main / a borrowed tail stream (-1: by size)
    char env_h_borrow = 0;                     // ZK_H_BORROW=a / l / b picks the borrowed stream (0: by entry point)
    char env_hl_tail = 0;                      // ZK_HL_TAIL=l / a: the merged H + L bucket reduction on the L- / A-tail stream instead of the H pipeline's (0)
    int env_b_tail_lanes = 0;                  // ZK_B_TAIL_LANES=1 / 4: lanes per point operation of the B-query's (G2) bucket reduction (0: by size / entry point)
    bool env_tails_on_acc = false;             // ZK_TAILS_ON_ACC=1: every bucket reduction on the accumulation stream, behind its accumulation (experiment)
    hipEvent_t ev_sort = nullptr;              // a finished bucket sort on s_main releases its accumulation on s_acc
    hipEvent_t ev_start = nullptr, ev_w = nullptr, ev_h = nullptr, ev_a0 = nullptr, ev_a1 = nullptr, ev_b0 = nullptr, ev_b1 = nullptr,
               ev_l0 = nullptr, ev_l1 = nullptr, ev_h1 = nullptr, ev_h0 = nullptr;
    ~zk_ctx() {
        set_in_flight(false);
        DeviceScope on(device);
        void *dev[] = {d_w, d_a, d_t, d_partials, d_bscale, d_hpart, d_tail};           // d_b, d_c live inside d_a's allocation
        for (void *p : dev) if (p) hipFree(p);
        if (h_w) hipHostFree(h_w);
        if (d_w2) hipFree(d_w2);
        if (h_w2) hipHostFree(h_w2);
        stream_park(s_copy, device, ROLE_COPY, stream_prio[ROLE_COPY]);
        if (ev_staged) hipEventDestroy(ev_staged);
        if (h_tail) hipHostFree(h_tail);
        cA.release(); cB.release(); cC.release();
        ntt_tables_free(tab);
        mA.release(); mH.release(); mL.release(); mB.release(); mW.release(); mB1.release();
        if (d_zk) hipFree(d_zk);
        if (ev_z1) hipEventDestroy(ev_z1);
        if (ev_z2) hipEventDestroy(ev_z2);
        if (ev_zf) hipEventDestroy(ev_zf);
        if (h_zk) { memset(h_zk, 0, (BLIND_RS_BYTES + BLIND_G1_BYTES + BLIND_G2_BYTES) * max_batch); hipHostFree(h_zk); }
        tables_release(tables);
        if (serial) s_a = s_b = s_l = nullptr;
        if (s_acc == s_main) s_acc = nullptr;
        if (ev_sort) hipEventDestroy(ev_sort);
        s_h = nullptr;                                   // never owned: s_main or s_l
        if (ev_up) hipEventDestroy(ev_up);
        if (ev_sort_h) hipEventDestroy(ev_sort_h);
        stream_park(s_main, device, ROLE_MAIN, stream_prio[ROLE_MAIN]); stream_park(s_acc, device, ROLE_ACC, stream_prio[ROLE_ACC]);
        stream_park(s_a, device, ROLE_A, stream_prio[ROLE_A]); stream_park(s_b, device, ROLE_B, stream_prio[ROLE_B]); stream_park(s_l, device, ROLE_L, stream_prio[ROLE_L]);
        hipEvent_t ee[] = {ev_start, ev_w, ev_h, ev_a0, ev_a1, ev_b0, ev_b1, ev_l0, ev_l1, ev_h1, ev_h0};
        for (auto e : ee) if (e) hipEventDestroy(e);
    }
};

extern "C" uint32_t zk_domain_size(uint32_t nC, uint32_t nIn) {
    uint32_t v = nC + nIn + 1;                                   // src/stubs.cpp:65
    v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; v++;   // roundUpToNearestPowerOf2, :49-59
    return v;
}

static int ctx_build(zk_ctx *c, const zk_pk *pk, const zk_csr *A, const zk_csr *B, const zk_csr *C) {
    ZK_TRY(use_device(c->device));
    const uint32_t m = c->m, V = c->V, nIn = c->nIn;
    const uint32_t G = c->cfg.shard_count > 1 ? c->cfg.shard_count : 1, r = G > 1 ? c->cfg.shard_rank : 0;
    c->rA = shard_range((uint32_t)pk->a_val.size(), r, G);
    c->rB = shard_range((uint32_t)pk->b_val.size(), r, G);
    // unsharded contexts with full tables prove with four transforms; ZK_SIX_TRANSFORMS=1 (read here, at context creation) keeps
    // the key's own H- and L-query bases and the six transforms
    const char *six = getenv("ZK_SIX_TRANSFORMS");
    const bool want_lag = G == 1 && !(six && six[0] && six[0] != '0');
    const uint64_t circ = want_lag ? csr_hash(C, nIn, V, m) : 0;
    auto set_ranges = [&](bool lag) {
        c->lag = lag; c->l_first = lag ? 0 : nIn + 1;
        c->rH = lag ? Range{0, m} : shard_range(m - 1, r, G);
        c->rL = lag ? Range{0, V + 1} : shard_range(V - nIn, r, G);
    };
    set_ranges(want_lag);
    {   // find or build the shared device tables of this (key, device, shard, window) combination
        std::lock_guard<std::mutex> lk(g_tables_mu);
        DeviceTables *t = nullptr;
        for (DeviceTables *e : g_tables)
            if (e->pk_id == pk->id && e->device == c->device && e->rank == r && e->count == G && e->cbits == c->cfg.multi_exp_c && e->max_batch == c->max_batch
                && e->lag_req == want_lag && e->circ == circ) { t = e; break; }
        if (!t) {
            std::unique_ptr<DeviceTables, DeviceTablesDeleter> fresh(new DeviceTables());      // (an error or exception below frees what was uploaded)
            t = fresh.get();
            t->pk_id = pk->id; t->device = c->device; t->rank = r; t->count = G; t->cbits = c->cfg.multi_exp_c; t->max_batch = c->max_batch;
            t->zk = pk->full && G == 1;                                 // (sharded contexts prove without zero knowledge only)
            t->lag_req = want_lag; t->circ = circ;
            // window bits, shared sort and table rows for the H- and L-query in the given bases
            auto plan_tables = [&](bool lag) {
                set_ranges(lag);
                t->lag = lag; t->plog = 0;
                // The A-, B- and L-query all read the witness: ONE bucket sort of the witness digits drives every query that is
                // dense in the window it covers.  Unsharded the window is the whole witness; a shard's window is the span of the
                // witness indices its three base ranges touch (base-range sharding cuts the three queries at about the same place).
                uint32_t lo = 0xffffffffu, hi = 0;
                auto span = [&](uint32_t first, uint32_t last) { if (first < lo) lo = first; if (last + 1 > hi) hi = last + 1; };
                if (c->rA.n()) span(pk->a_idx[c->rA.lo], pk->a_idx[c->rA.hi - 1]);
                if (c->rB.n()) span(pk->b_idx[c->rB.lo], pk->b_idx[c->rB.hi - 1]);
                if (c->rL.n()) span(c->l_first + c->rL.lo, c->l_first + c->rL.hi - 1);
                if (G == 1) { lo = 0; hi = V + 1; }
                if (lo > hi) lo = hi = 0;
                t->win_lo = lo; t->win_n = hi - lo;
                const uint64_t dense = (uint64_t)t->win_n * 7 / 8;
                const bool can_share = t->win_n >= 64 && !getenv("ZK_NO_SHARED_SORT");
                t->share_A = can_share && c->rA.n() >= dense;
                t->share_B = can_share && c->rB.n() >= dense;
                t->share_L = can_share && c->rL.n() >= dense;
                if ((int)t->share_A + (int)t->share_B + (int)t->share_L < 2) t->share_A = t->share_B = t->share_L = false;   // nothing to share
                auto window = [&](uint32_t n) { return t->cbits ? t->cbits : MsmShape::pick_c(n ? n : 1, t->max_batch); };
                t->cW = window(t->win_n);
                t->cA = t->share_A ? t->cW : window(c->rA.n()); t->cB = t->share_B ? t->cW : window(c->rB.n());
                t->cH = window(c->rH.n()); t->cL = t->share_L ? t->cW : window(c->rL.n());
                {   // make room for this key's tables (5 GB at 2^20, 20 GB at 2^22): idle table sets on this device go first.  If the tables still
                    // do not fit they keep every 2nd, 4th, ... window only (MsmShape::plog: S bucket planes, c S doublings between table rows, the
                    // planes folded on the host) instead of failing the context: the reference's domain goes up to 2^28 (src/stubs.cpp:49-75),
                    // whose full tables would be 16 x the key.  ZK_TABLE_BUDGET=<bytes> (read here, at context creation) stands in for the free
                    // memory: a test aid, and a way to leave room for other tenants of the device.
                    auto rows_of = [&](uint32_t cb, uint32_t plog) { const uint32_t W = 254 / cb + 1, S = 1u << plog; return (uint64_t)((W + S - 1) >> plog); };
                    auto bytes_at = [&](uint32_t plog) {
                        return 64ull * (rows_of(t->cA, plog) * c->rA.n() + rows_of(t->cH, plog) * c->rH.n() + rows_of(t->cL, plog) * c->rL.n()) + 128ull * rows_of(t->cB, plog) * c->rB.n()
                               + (t->zk ? 64ull * rows_of(t->cB, plog) * c->rB.n() + (64ull + 128ull) * BLIND_ROWS : 0);   // a zero-knowledge context: B1, delta1, delta2
                    };
                    t->full_table_bytes = bytes_at(0);
                    // what a context needs beside the tables: sort scratch (12 B per entry, two sorts), chunk pieces, polynomials, CSR -- about 16 B per
                    // entry of the four queries plus 8 GB of slack (the figure the eviction loop always kept)
                    const uint64_t entries = 15ull * ((uint64_t)c->rA.n() + c->rB.n() * (t->zk ? 2 : 1) + c->rH.n() + c->rL.n()) * c->max_batch;   // (B1: reduction buffers of its own)
                    const uint64_t reserve = (8ull << 30) + 16ull * entries;
                    size_t mem_free = 0, mem_total = 0;
                    while (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && t->full_table_bytes + reserve > mem_free && tables_evict_idle_locked(c->device)) {}
                    uint64_t budget = mem_free > reserve ? mem_free - reserve : 0;
                    if (const char *e = getenv("ZK_TABLE_BUDGET")) budget = strtoull(e, nullptr, 10);
                    // (proofs x planes x buckets must fit the sort's 2^20 bucket ids: MsmWork::alloc checks the same)
                    const uint32_t cmax = std::max(std::max(t->cA, t->cB), std::max(t->cH, t->cL));
                    auto sets_fit = [&](uint32_t plog) { return (((uint64_t)c->max_batch << plog) << (cmax - 1)) <= (1ull << 20); };
                    while (bytes_at(t->plog) > budget && t->plog < 4 && sets_fit(t->plog + 1)) t->plog++;
                    t->table_bytes = bytes_at(t->plog);
                }
            };
            plan_tables(want_lag);
            if (t->lag && t->plog) plan_tables(false);               // the Lagrange tables would come out frugal: the key's own bases, six transforms
            int rc = dev_upload(&t->dA_idx, pk->a_idx.data() + c->rA.lo, c->rA.n());
            if (rc == ZK_OK) rc = dev_upload(&t->dB_idx, pk->b_idx.data() + c->rB.lo, c->rB.n());
            // window position -> shard entry: consecutive indices need no map (entry = position - off), else an explicit one
            auto inverse = [&](const std::vector<uint32_t> &idx, Range r, uint32_t **out, uint32_t *off) -> int {
                *out = nullptr; *off = 0;
                if (!r.n()) return ZK_OK;
                bool run = true;
                for (uint32_t k = r.lo; k < r.hi && run; k++) run = idx[k] == idx[r.lo] + (k - r.lo);
                if (run) { *off = idx[r.lo] - t->win_lo; return ZK_OK; }
                std::vector<uint32_t> pos(t->win_n, 0xffffffffu);
                for (uint32_t k = r.lo; k < r.hi; k++) pos[idx[k] - t->win_lo] = k - r.lo;
                return dev_upload(out, pos.data(), pos.size());
            };
            if (rc == ZK_OK && t->share_A) rc = inverse(pk->a_idx, c->rA, &t->posA, &t->offA);
            if (rc == ZK_OK && t->share_B) rc = inverse(pk->b_idx, c->rB, &t->posB, &t->offB);
            t->offL = c->rL.n() ? c->l_first + c->rL.lo - t->win_lo : 0;
            if (rc == ZK_OK) rc = build_table<G1>(&t->tA, pk->a_val.data() + c->rA.lo, c->rA.n(), t->cA, t->plog);
            if (rc == ZK_OK && t->lag) {                                 // Q_j and L_v - K_v instead of the key's H- and L-query (hlagrange.hpp)
                const double t0 = now_ms();
                DevScratch s;
                G1::Affine *d_q = nullptr, *d_lk = nullptr;
                rc = s.get(&d_q, m);
                if (rc == ZK_OK) rc = s.get(&d_lk, (size_t)V + 1);
                if (rc == ZK_OK) rc = hl_transform_bases(pk->H.data(), pk->L.data(), C, c->logm, nIn, V, d_q, d_lk);
                t->lag_ms = now_ms() - t0;                              // (hl_transform_bases ends with a device synchronisation)
                if (rc == ZK_OK) rc = build_table_dev<G1>(&t->tH, d_q, m, t->cH, t->plog);
                if (rc == ZK_OK) rc = build_table_dev<G1>(&t->tL, d_lk, V + 1, t->cL, t->plog);
            } else {
            if (rc == ZK_OK) rc = build_table<G1>(&t->tH, pk->H.data() + c->rH.lo, c->rH.n(), t->cH, t->plog);
            if (rc == ZK_OK) rc = build_table<G1>(&t->tL, pk->L.data() + c->rL.lo, c->rL.n(), t->cL, t->plog);
            }
            if (rc == ZK_OK) rc = build_table<G2>(&t->tB, pk->b_val.data() + c->rB.lo, c->rB.n(), t->cB, t->plog);
            if (rc == ZK_OK && t->zk) {
                if (pk->b1_val.size() != pk->b_val.size()) rc = fail(ZK_ERR_ARG, "full key: the G1 half of the B-query has another length than the G2 half");
                if (rc == ZK_OK) rc = build_table<G1>(&t->tB1, pk->b1_val.data() + c->rB.lo, c->rB.n(), t->cB, t->plog);
                std::vector<G1::Affine> d1; std::vector<G2::Affine> d2;
                if (rc == ZK_OK) { blind_table_host<G1>(pk->delta_g1, d1); rc = dev_upload(&t->tD1, d1.data(), d1.size()); }
                if (rc == ZK_OK) { blind_table_host<G2>(pk->delta_g2, d2); rc = dev_upload(&t->tD2, d2.data(), d2.size()); }
            }
            if (rc != ZK_OK) return rc;
            g_tables.push_back(t);
            fresh.release();
        }
        t->refs++;
        c->tables = t;
        set_ranges(t->lag);
    }
    c->dA_idx = c->tables->dA_idx; c->dB_idx = c->tables->dB_idx;
    const DeviceTables *t = c->tables;
    const bool any_share = t->share_A || t->share_B || t->share_L;
    const uint32_t KB = c->max_batch;
    if (any_share) { ZK_TRY(c->mW.alloc(t->win_n, t->cW, nullptr, nullptr, /*sort_only=*/true, KB, t->plog)); c->mW.use_shift_payload(); }
    ZK_TRY(c->mA.alloc(c->rA.n(), t->cA, t->tA, t->share_A ? &c->mW.sh : nullptr, false, KB, t->plog));
    ZK_TRY(c->mH.alloc(c->rH.n(), t->cH, t->tH, nullptr, false, KB, t->plog));
    ZK_TRY(c->mL.alloc(c->rL.n(), t->cL, t->tL, t->share_L ? &c->mW.sh : nullptr, false, KB, t->plog));
    ZK_TRY(c->mB.alloc(c->rB.n(), t->cB, t->tB, t->share_B ? &c->mW.sh : nullptr, false, KB, t->plog));
    if (t->zk) {       // B1: the B-query's shape and sort (the shared witness sort, or mB's own), G1 accumulation and tail; blinding buffers
        ZK_TRY(c->mB1.alloc(c->rB.n(), t->cB, t->tB1, t->share_B ? &c->mW.sh : &c->mB.sh, false, KB, t->plog));
        const size_t per = BLIND_RS_BYTES + BLIND_G1_BYTES + BLIND_G2_BYTES;
        ZK_HIP(hipMalloc(&c->d_zk, (per + BLIND_FIX_BYTES) * KB));
        ZK_HIP(hipHostMalloc(&c->h_zk, per * KB, hipHostMallocDefault));
        memset(c->h_zk, 0, per * KB);
        ZK_HIP(hipEventCreate(&c->ev_z1)); ZK_HIP(hipEventCreate(&c->ev_z2));
        ZK_HIP(hipEventCreateWithFlags(&c->ev_zf, hipEventDisableTiming));
        c->beta_g1 = pk->beta_g1;
    }
    ZK_TRY(c->cA.upload(A, V, KB)); ZK_TRY(c->cB.upload(B, V, KB)); ZK_TRY(c->cC.upload(C, V, KB));
    ZK_HIP(hipMalloc(&c->d_w, 32 * (size_t)(V + 1) * KB));
    // A | B | C polynomials of all proofs of a batch: [A: KB x m][B: KB x m][C: KB x m], one batched NTT launch per pass
    ZK_HIP(hipMalloc(&c->d_a, 3 * 32 * (size_t)m * KB)); c->d_b = c->d_a + (size_t)m * KB; c->d_c = c->d_a + 2 * (size_t)m * KB;
    ZK_HIP(hipMalloc(&c->d_t, 3 * 32 * (size_t)m * KB));
    ZK_HIP(hipMalloc(&c->d_partials, sizeof(zk_partials) * KB));
    ZK_HIP(hipMemset(c->d_partials, 0, sizeof(zk_partials) * KB));                  // (a merged H + L tail never writes Lt: it stays the point at infinity)
    c->merge_hl = c->rH.n() && c->rL.n() && c->mH.sh.nb == c->mL.sh.nb && c->mH.sh.plog == c->mL.sh.plog && !getenv("ZK_NO_MERGE_HL");
    if (G > 1) {      // sharded provers exchange the device copy of their partial sums (zk_prove_collect_device)
        c->mA.dev_result = (G1::XYZZ *)(c->d_partials + offsetof(zk_partials, At)); c->mB.dev_result = (G2::XYZZ *)(c->d_partials + offsetof(zk_partials, Bt));
        c->mH.dev_result = (G1::XYZZ *)(c->d_partials + offsetof(zk_partials, Ht));
        if (!c->merge_hl) c->mL.dev_result = (G1::XYZZ *)(c->d_partials + offsetof(zk_partials, Lt));
    }
    c->mA.dev_result_pitch = c->mB.dev_result_pitch = c->mH.dev_result_pitch = c->mL.dev_result_pitch = sizeof(zk_partials);
    ZK_HIP(hipHostMalloc(&c->h_w, 32 * (size_t)(V + 1) * KB, hipHostMallocDefault));
    ZK_HIP(hipHostMalloc(&c->h_tail, 32 * (size_t)KB, hipHostMallocDefault));
    if (c->lag) {
        ZK_HIP(hipMalloc(&c->d_bscale, 32 * (size_t)m));
        ZK_HIP(hipMalloc(&c->d_hpart, 2 * 32 * (size_t)zk_div_up(m, HL_PROD_THREADS) * KB));
        ZK_HIP(hipMalloc(&c->d_tail, 32 * (size_t)KB));
    }
    // s_main (high priority) carries the short memory- and latency-bound kernels: witness upload, bucket sorts, the H
    // polynomial pipeline; s_acc (low priority) carries the four machine-filling accumulation kernels, each released by
    // the event of its sort; the bucket-reduction tails run on side streams.  The priorities make the dispatcher hand freed
    // wave slots to the short kernels first, so the H pipeline advances in the shadow of the A-, B-, L-accumulations of the
    // same proof instead of queueing behind them.  zk_config.schedule = ZK_SCHED_ONE_STREAM (or ZK_SERIAL=1) puts everything on s_main;
    // ZK_SPLIT_STREAMS=0 keeps the accumulations on s_main as well (the round-1 schedule).
    int prio_lo = 0, prio_hi = 0;
    ZK_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    // stream priorities, in the order main, accumulate, A-tail, B-tail, L-tail: h(igh) / n(ormal) / l(ow).  Measured at 2^20 with
    // three proofs in flight (profiles/r02_stream_priorities.txt): the accumulations and the A- / L-tails low, the rest high is
    // the best of the combinations tried; every tail high costs 12 % (their few, register-heavy waves push accumulation waves out).
    // zk_config.schedule = ZK_SCHED_LATENCY (a context that proves one synchronous proof at a time: ethsnarks::prove): every stream at the
    // same priority for circuits past the small-proof schedule.  How the runtime spreads a context's streams over its hardware queues (a
    // pool of GPU_MAX_HW_QUEUES = 4 per priority) decides how fast the proof's ~25 short kernels get dispatched beside its four long ones:
    // synchronous zk_prove, mixed -> all high: 2^16 1.99 -> 1.62 ms, 2^18 3.68 -> 3.38, 2^20 10.52 -> 10.22; the small circuits (Merkle-29
    // 1.18 -> 1.39, 2^14 1.23 -> 1.34) and pipelined contexts (2^18: 306 -> 275 proofs/s) want the mixed priorities
    // (tools/dev_queue_map.py, tools/dev_sync_latency.py; profiles/r03_queue_mapping.txt).
    const bool latency_sched = c->cfg.schedule == ZK_SCHED_LATENCY && (uint64_t)c->mH.sh.max_entries() * c->max_batch >= (3ull << 18);
    const char *pr = getenv("ZK_PRIOS");                              // tuning aid
    if (!pr || strlen(pr) != 5) pr = latency_sched ? "hhhhh" : "hllhl";
    auto prio = [&](char ch) { return ch == 'h' ? prio_hi : ch == 'l' ? prio_lo : (prio_hi + prio_lo) / 2; };
    for (int i = 0; i < 5; i++) c->stream_prio[i] = prio(pr[i]);
    ZK_TRY(stream_take(&c->s_main, c->device, ROLE_MAIN, c->stream_prio[ROLE_MAIN]));
    c->env_no_direct_h2d = getenv("ZK_NO_DIRECT_H2D") != nullptr;
    if (const char *e = getenv("ZK_H_STREAM")) c->env_h_stream = e[0] == '1' ? 1 : 0;
    if (const char *e = getenv("ZK_H_BORROW")) c->env_h_borrow = e[0];
    if (const char *e = getenv("ZK_HL_TAIL")) c->env_hl_tail = e[0];
    if (const char *e = getenv("ZK_B_TAIL_LANES")) c->env_b_tail_lanes = atoi(e);
    c->env_tails_on_acc = getenv("ZK_TAILS_ON_ACC") != nullptr;
    const char *serial = getenv("ZK_SERIAL");
    c->serial = (serial && serial[0] == '1') || c->cfg.schedule == ZK_SCHED_ONE_STREAM;
    const char *split = getenv("ZK_SPLIT_STREAMS");
    if (c->serial || (split && split[0] == '0')) c->s_acc = c->s_main;
    else ZK_TRY(stream_take(&c->s_acc, c->device, ROLE_ACC, c->stream_prio[ROLE_ACC]));
    ZK_HIP(hipEventCreate(&c->ev_sort));
    c->s_h = c->s_main;                                               // small proofs move the H pipeline to a tail stream (prove_enqueue)
    if (c->serial) { c->s_a = c->s_b = c->s_l = c->s_main; }
    else {
        ZK_TRY(stream_take(&c->s_a, c->device, ROLE_A, c->stream_prio[ROLE_A]));
        ZK_TRY(stream_take(&c->s_b, c->device, ROLE_B, c->stream_prio[ROLE_B]));
        ZK_TRY(stream_take(&c->s_l, c->device, ROLE_L, c->stream_prio[ROLE_L]));
    }
    hipEvent_t *ee[] = {&c->ev_start, &c->ev_w, &c->ev_h, &c->ev_a0, &c->ev_a1, &c->ev_b0, &c->ev_b1, &c->ev_l0, &c->ev_l1, &c->ev_h1, &c->ev_h0};
    for (auto e : ee) ZK_HIP(hipEventCreate(e));
    ZK_TRY(ntt_tables_create(c->tab, c->logm, c->s_main));
    if (c->lag) {
        const fe g = Fr::from_u64(5), mi = Fr::inv(Fr::from_u64(m)), mz = Fr::mul(mi, c->tab.zinv);
        ZK_LAUNCH(k_fill_geometric, zk_div_up(zk_div_up(m, 256), 64), 64, c->s_main, c->d_bscale, m, g, Fr::from_mont(mi));   // g^i / (m R)
        c->hl_kp = Fr::to_mont(Fr::mul(mz, Fr::inv(Fr::pow_u64(g, m - 1))));                                                  // R^2 g^-(m-1) / (m Z(g))
        c->hl_kc = mz;
        c->hl_zg = Fr::sub(Fr::pow_u64(g, m), Fr::one());
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipStreamSynchronize(c->s_main));
    return ZK_OK;
}

extern "C" int zk_ctx_create(const zk_pk *pk, const zk_csr *A, const zk_csr *B, const zk_csr *C,
                             uint32_t nC, uint32_t nIn, uint32_t V, const zk_config *cfg, zk_ctx **out) try {
    if (!pk || !A || !B || !C || !out) return fail(ZK_ERR_ARG, "null argument");
    if (A->n_rows != nC || B->n_rows != nC || C->n_rows != nC) return fail(ZK_ERR_ARG, "CSR row counts must equal nC");
    if (nIn > V) return fail(ZK_ERR_ARG, "nIn > V");
    if ((uint64_t)nC + nIn + 1 > (1ull << 28)) return fail(ZK_ERR_ARG, "domain exceeds 2^28 (2-adicity of r - 1)");
    const uint32_t m = zk_domain_size(nC, nIn);
    // the reference's DEBUG asserts, tcc:477-483, made unconditional
    if (pk->a_domain != V + 1 || pk->b_domain != V + 1 || pk->H.size() != (size_t)m - 1 || pk->L.size() != (size_t)(V - nIn))
        return fail(ZK_ERR_SHAPE, "proving key shape does not match (A/B domain = V+1, |H| = m-1, |L| = V-nIn)");
    std::unique_ptr<zk_ctx> holder(new zk_ctx());           // (whatever ends the construction early -- error code or exception -- releases it)
    zk_ctx *c = holder.get();
    if (cfg) c->cfg = *cfg;
    if (c->cfg.shard_count > 1 && c->cfg.shard_rank >= c->cfg.shard_count) return fail(ZK_ERR_ARG, "shard_rank >= shard_count");
    c->device = (int)c->cfg.device;
    c->max_batch = c->cfg.max_batch ? c->cfg.max_batch : 1;
    if (c->max_batch > 4096) return fail(ZK_ERR_ARG, "max_batch > 4096");
    c->nC = nC; c->nIn = nIn; c->V = V; c->m = m;
    while ((1u << c->logm) < m) c->logm++;
    c->alpha_g1 = pk->alpha_g1; c->beta_g2 = pk->beta_g2;
    ZK_TRY(ctx_build(c, pk, A, B, C));
    *out = holder.release();
    return ZK_OK;
} ZK_GUARD
// clients built against another layout of zk_config pass the size THEY know: missing trailing members read as 0 (their defaults)
extern "C" int zk_ctx_create_sized(const zk_pk *pk, const zk_csr *A, const zk_csr *B, const zk_csr *C,
                                   uint32_t nC, uint32_t nIn, uint32_t V, const zk_config *cfg, size_t cfg_size, zk_ctx **out) try {
    zk_config full{};
    if (cfg) memcpy(&full, cfg, cfg_size < sizeof(full) ? cfg_size : sizeof(full));
    return zk_ctx_create(pk, A, B, C, nC, nIn, V, cfg ? &full : nullptr, out);
} ZK_GUARD
extern "C" void zk_ctx_destroy(zk_ctx *ctx) try { delete ctx; } ZK_GUARD_VOID

// ---- the row evaluations of the k = cur_batch witnesses in d_w: [A: k x m][B: k x m][C: k x m] in d_a, Montgomery; the row kernels write the
// padding and A's input-consistency rows too.  Both H pipelines start with it, and zk_ctx_probe_rows is nothing else.
static int enqueue_rows(zk_ctx *c, hipStream_t st) {
    const uint32_t m = c->m, k = c->cur_batch, ws = c->V + 1;
    fe *a = c->d_a, *b = c->d_a + (size_t)m * k, *cc = c->d_a + 2 * (size_t)m * k;
    ZK_TRY(c->cA.enqueue(c->d_w, a, st, k, ws, m, m, c->nIn + 1));
    ZK_TRY(c->cB.enqueue(c->d_w, b, st, k, ws, m, m, 0));
    ZK_TRY(c->cC.enqueue(c->d_w, cc, st, k, ws, m, m, 0));
    return ZK_OK;
}

// TEST INFRASTRUCTURE (zk_ctx_probe_h): host buffers that receive what each step of an H pipeline left, through stream-ordered copies enqueued
// BETWEEN its launches (the steps overwrite each other's buffers).  The proving path passes none: same kernels, arguments and order.
struct HSnap { fe *first, *coset, *last, *hpart, *tail; };
static int h_snapshot(const HSnap *snap, fe *HSnap::*which, const fe *d_src, size_t n, hipStream_t st) {
    if (snap && snap->*which) ZK_HIP(hipMemcpyAsync(snap->*which, d_src, 32 * n, hipMemcpyDeviceToHost, st));
    return ZK_OK;
}

// ---- "Compute the polynomial H" (tcc:460-475) on s_main; result in d_t (natural order), h[m-1] copied to h_tail
// for the k = cur_batch proofs in flight: polynomials laid out [A: k x m][B: k x m][C: k x m] in d_a, h of proof p at d_t + p m
static int enqueue_compute_h(zk_ctx *c, hipStream_t st, const HSnap *snap = nullptr) {
    const uint32_t m = c->m, k = c->cur_batch;
    fe *a = c->d_a, *b = c->d_a + (size_t)m * k, *cc = c->d_a + 2 * (size_t)m * k;
    ZK_TRY(enqueue_rows(c, st));
    // all 3 k polynomials go through each pass together (blockIdx.y): fewer, larger launches
    // SIX transforms, not the reference's seven (libsnark: iFFT and cosetFFT of A, B and C, divide by Z on the coset, icosetFFT): C never
    // goes to the coset.  With P = A B, icosetFFT(P on the coset) is P mod (x^m - g^m) = Z(g) H + C for every witness (deg H, deg C < m,
    // Z = x^m - 1, Z on the coset is the constant Z(g) = g^m - 1), so  h = icosetFFT(A B) / Z(g) - C / Z(g):  the same field elements
    // (the coefficients are unique), one forward transform and one pass over four vectors less.  The product A B is formed when the
    // last transform loads its input, C / Z(g) comes out of its iFFT (scaled there) and is subtracted when the last transform stores.
    (void)cc;
    NttFuse cscale; cscale.post_alt = c->tab.inv_m_zinv; cscale.alt_from = 2 * k;                     // vectors [2k, 3k) are the C polynomials
    ZK_TRY(ntt_run(c->tab, a, c->d_t, true, nullptr, c->tab.inv_then_coset, st, 3 * k, m, cscale));   // iFFT of A, B (x g^i / m: cosetFFT pre-scale) and of C (x 1 / (m Z(g)))
    if (snap) ZK_TRY(h_snapshot(snap, &HSnap::first, c->d_t, 3 * (size_t)m * k, st));
    ZK_TRY(ntt_run(c->tab, c->d_t, a, false, nullptr, nullptr, st, 2 * k, m));                        // FFT: A, B on the coset
    if (snap) ZK_TRY(h_snapshot(snap, &HSnap::coset, a, 2 * (size_t)m * k, st));
    NttFuse last; last.in2 = b; last.sub = c->d_t + 2 * (size_t)m * k;
    ZK_TRY(ntt_run(c->tab, a, c->d_t, true, nullptr, c->tab.icoset_zinv, st, k, m, last));            // icosetFFT of A B, / Z(g), - C / Z(g)
    if (snap) ZK_TRY(h_snapshot(snap, &HSnap::last, c->d_t, (size_t)m * k, st));
    if (k == 1) ZK_HIP(hipMemcpyAsync(c->h_tail, c->d_t + (m - 1), 32, hipMemcpyDeviceToHost, st));
    else ZK_HIP(hipMemcpy2DAsync(c->h_tail, 32, c->d_t + (m - 1), 32 * (size_t)m, 32, k, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// ---- the same for a context whose H-query lies in coset-Lagrange bases (hlagrange.hpp): FOUR transforms.  The H scalars are the
// products p_j = A(g w^j) B(g w^j), canonical, in d_t (proof p at d_t + p m); the C row evaluations are scalars of nothing -- their part of h
// is in the L-query's bases -- and only enter the degree check: h[m-1] as a dot product over p and c, copied to h_tail as above.
static int enqueue_compute_h4(zk_ctx *c, hipStream_t st, const HSnap *snap = nullptr) {
    const uint32_t m = c->m, k = c->cur_batch;
    fe *a = c->d_a, *b = c->d_a + (size_t)m * k, *cc = c->d_a + 2 * (size_t)m * k;
    ZK_TRY(enqueue_rows(c, st));
    NttFuse bscale; bscale.post_alt = c->d_bscale; bscale.alt_from = k;                                 // vectors [k, 2k) are the B polynomials: x 1 / R as well
    ZK_TRY(ntt_run(c->tab, a, c->d_t, true, nullptr, c->tab.inv_then_coset, st, 2 * k, m, bscale));   // iFFT of A, B (x g^i / m: cosetFFT pre-scale)
    if (snap) ZK_TRY(h_snapshot(snap, &HSnap::first, c->d_t, 2 * (size_t)m * k, st));
    ZK_TRY(ntt_run(c->tab, c->d_t, a, false, nullptr, nullptr, st, 2 * k, m));                        // FFT: A, B on the coset
    if (snap) ZK_TRY(h_snapshot(snap, &HSnap::coset, a, 2 * (size_t)m * k, st));
    const uint32_t grid = zk_div_up(m, HL_PROD_THREADS * HL_PROD_PER);
    ZK_LAUNCH_SYNC(k_hl_product, dim3(grid, k), HL_PROD_THREADS, st, (const fe *)a, (const fe *)b, (const fe *)cc, (const fe *)c->tab.tw_fwd, c->d_t, c->d_hpart, m, m);
    if (snap) { ZK_TRY(h_snapshot(snap, &HSnap::last, c->d_t, (size_t)m * k, st)); ZK_TRY(h_snapshot(snap, &HSnap::hpart, c->d_hpart, 2 * (size_t)grid * k, st)); }
    ZK_LAUNCH_SYNC(k_hl_tail, k, HL_PROD_THREADS, st, (const fe *)c->d_hpart, grid, c->hl_kp, c->hl_kc, c->d_tail);
    if (snap) ZK_TRY(h_snapshot(snap, &HSnap::tail, c->d_tail, k, st));
    ZK_HIP(hipMemcpyAsync(c->h_tail, c->d_tail, 32 * (size_t)k, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// ... and for an h that arrives as coefficients (zk_prove_submit_h, zk_prove_submit_with_h: the two-step submit, whose h comes from the
// six-transform chains): p = cosetFFT(Z(g) h + C), C's coefficients from its row evaluations -- two transforms on a path that is rare on an
// unsharded context.  One proof; d_h may be the context's own d_t.  Result in d_t, Montgomery.
static int enqueue_h_coefficients_to_coset(zk_ctx *c, const fe *d_h, hipStream_t st) {
    const uint32_t m = c->m, ws = c->V + 1;
    fe *cc = c->d_a + 2 * (size_t)m, *ccoef = c->d_t + 2 * (size_t)m;
    ZK_TRY(c->cC.enqueue(c->d_w, cc, st, 1, ws, m, m, 0));
    ZK_TRY(ntt_run(c->tab, cc, ccoef, true, nullptr, c->tab.inv_m, st));
    ZK_LAUNCH(k_hl_q_from_h, zk_div_up(m, 256), 256, st, d_h, m - 1, (const fe *)ccoef, c->hl_zg, c->d_a, m);
    ZK_TRY(ntt_run(c->tab, c->d_a, c->d_t, false, c->tab.coset_fwd, nullptr, st));
    return ZK_OK;
}

// ---- SURVEY 8(e) option 2 (sharded latency mode): the A, B and C transform chains of the witness map on three different
// ranks.  One chain = row evaluations of one matrix, iFFT, cosetFFT; its m coset evaluations stay in d_a + which * m.
static int enqueue_chain(zk_ctx *c, int which) {
    hipStream_t st = c->s_main;
    const uint32_t m = c->m, ws = c->V + 1;
    fe *p = c->d_a + (size_t)which * m, *tmp = c->d_t + (size_t)which * m;
    const DevCsr &M = which == 0 ? c->cA : which == 1 ? c->cB : c->cC;
    ZK_TRY(M.enqueue(c->d_w, p, st, 1, ws, m, m, which == 0 ? c->nIn + 1 : 0));
    if (which == 2) return ntt_run(c->tab, p, tmp, true, nullptr, c->tab.inv_m_zinv, st);      // C stays in coefficient form, / Z(g) (enqueue_compute_h): at d_t + 2 m
    ZK_TRY(ntt_run(c->tab, p, tmp, true, nullptr, c->tab.inv_then_coset, st));
    ZK_TRY(ntt_run(c->tab, tmp, p, false, nullptr, nullptr, st));
    return ZK_OK;
}
// h from the three chains (device pointers, m elements each; they may live anywhere in this device's memory): result in d_t
static int enqueue_h_from_chains(zk_ctx *c, const fe *a, const fe *b, const fe *cc) {
    hipStream_t st = c->s_main;
    const uint32_t m = c->m;
    if (cc >= c->d_t && cc < c->d_t + m) return fail(ZK_ERR_ARG, "zk_h_from_chains_submit: the C chain overlaps the context's h buffer");
    NttFuse last; last.in2 = b; last.sub = cc;                      // a, b: coset evaluations; cc: coefficients of C / Z(g)
    ZK_TRY(ntt_run(c->tab, a, c->d_t, true, nullptr, c->tab.icoset_zinv, st, 1, m, last));
    ZK_HIP(hipMemcpyAsync(c->h_tail, c->d_t + (m - 1), 32, hipMemcpyDeviceToHost, st));
    return ZK_OK;
}

// witness: a host buffer (staged through pinned memory, the reference's pb.values), or -- resident != 0 -- a buffer that
// already lives in this device's memory (the caller keeps it untouched until the proof is collected)
// resident: 0 = host buffer, 1 = device buffer of the caller, 2 = staged earlier (zk_prove_stage): already in d_w,
//           3 = PINNED host buffer of the caller (zk_host_alloc / zk_host_register): copied from where it lies, no staging
static int upload_witness(zk_ctx *c, const uint64_t *witness, int canonical, int resident = 0) {
    const size_t n = (size_t)(c->V + 1) * c->cur_batch;          // the witnesses of a batch are contiguous
    // a queued proof copies the caller's buffer into pinned memory (the caller may reuse it at once, the H2D copy is asynchronous);
    // a synchronous call hands the caller's buffer to the runtime, which pipelines its own staging with the DMA
    const bool direct = resident == 3 || (!resident && c->latency_call && !c->env_no_direct_h2d);
    if (resident == 3) resident = 0;
    if (!resident && !direct) memcpy(c->h_w, witness, 32 * n);
    if (resident == 2) ZK_HIP(hipStreamWaitEvent(c->s_main, c->ev_staged, 0));
    ZK_HIP(hipEventRecord(c->ev_start, c->s_main));
    if (resident == 1) ZK_HIP(hipMemcpyAsync(c->d_w, witness, 32 * n, hipMemcpyDeviceToDevice, c->s_main));
    else if (direct) ZK_HIP(hipMemcpyAsync(c->d_w, witness, 32 * n, hipMemcpyHostToDevice, c->s_main));
    else if (!resident) ZK_HIP(hipMemcpyAsync(c->d_w, c->h_w, 32 * n, hipMemcpyHostToDevice, c->s_main));
    if (canonical) ZK_LAUNCH(k_to_mont, zk_div_up(n, 256), 256, c->s_main, c->d_w, (uint32_t)n);
    ZK_HIP(hipEventRecord(c->ev_w, c->s_main));
    return ZK_OK;
}

static void store_xyzz(uint64_t *dst, const G1::XYZZ &p) { memcpy(dst, &p, sizeof(p)); }
static void store_xyzz(uint64_t *dst, const G2::XYZZ &p) { memcpy(dst, &p, sizeof(p)); }

// phase: PHASE_ALL = the whole proof; PHASE_WITNESS = everything that needs only the witness (upload, witness sorts, A-, B-, L-query);
// PHASE_H = the H-query of a proof whose witness part is already queued (its coefficients come from d_h)
enum { PHASE_ALL = 0, PHASE_WITNESS = 1, PHASE_H = 2 };
static int prove_enqueue(zk_ctx *c, const uint64_t *witness, int canonical, int resident, const fe *d_h, int phase);
static void zk_clear_rs(zk_ctx *c);
static void drain(zk_ctx *c) {
    c->mL.tail_pending = c->mH.tail_pending = c->mB1.tail_pending = false;            // (a dropped proof's chunk pieces are not folded into the next one's reduction)
    hipStreamSynchronize(c->s_main); hipStreamSynchronize(c->s_acc); hipStreamSynchronize(c->s_a); hipStreamSynchronize(c->s_b); hipStreamSynchronize(c->s_l); hipStreamSynchronize(c->s_h);
}
static int prove_submit_impl(zk_ctx *c, const uint64_t *witness, int canonical, int resident = 0, uint32_t k = 1, const fe *d_h = nullptr, int phase = PHASE_ALL) {
    if (!c || (!witness && phase != PHASE_H)) return fail(ZK_ERR_ARG, "null argument");
    if (phase == PHASE_H) {
        if (!c->in_flight || !c->awaiting_h) return fail(ZK_ERR_ARG, "zk_prove_submit_h: no proof is waiting for its H part on this context (zk_prove_submit_defer_h first)");
        if (!d_h) return fail(ZK_ERR_ARG, "null argument");
    } else if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is already in flight on this context (collect it first)");
    if (!k || k > c->max_batch) return fail(ZK_ERR_ARG, "batch size exceeds zk_config.max_batch of this context");
    ZK_TRY(use_device(c->device));
    if (phase != PHASE_H) c->cur_batch = k;
    const int rc = prove_enqueue(c, witness, canonical, resident, d_h, phase);
    if (rc != ZK_OK) {      // part of the proof may be queued: drain it so that the next submit cannot overwrite buffers still in use
        drain(c);
        c->set_in_flight(false); c->awaiting_h = false;
        return rc;
    }
    c->set_in_flight(true);
    c->awaiting_h = phase == PHASE_WITNESS;
    return ZK_OK;
}
// d_h != nullptr: the H polynomial was computed elsewhere (option 2); this shard's coefficients [rH.lo, rH.hi) lie at d_h
static int prove_enqueue(zk_ctx *c, const uint64_t *witness, int canonical, int resident, const fe *d_h, int phase) {
    const bool zk = c->cur_zk && phase == PHASE_ALL;
    const size_t zk_g1_at = BLIND_RS_BYTES * c->max_batch, zk_g2_at = zk_g1_at + BLIND_G1_BYTES * c->max_batch,
                 zk_fix_at = zk_g2_at + BLIND_G2_BYTES * c->max_batch;
    if (zk) ZK_HIP(hipMemcpyAsync(c->d_zk, c->h_zk, BLIND_RS_BYTES * c->cur_batch, hipMemcpyHostToDevice, c->s_main));   // r, s: before the upload (ev_w) and every sort
    if (phase != PHASE_H) ZK_TRY(upload_witness(c, witness, canonical, resident));
    if (zk) {       // r delta1, s delta1, -rs delta1 need no MSM result: on the B-tail stream, idle until the B-query's tail
        ZK_HIP(hipStreamWaitEvent(c->s_b, c->ev_w, 0));
        ZK_LAUNCH(k_zk_blind_fixed, zk_div_up((uint64_t)c->cur_batch * 3 * BLIND_Q, BLIND_BLOCK), BLIND_BLOCK, c->s_b, (const G1::Affine *)c->tables->tD1,
                  (const fe *)c->d_zk, (G1::XYZZ *)(c->d_zk + zk_fix_at), c->cur_batch);
        ZK_HIP(hipEventRecord(c->ev_zf, c->s_b));
    }
    // sorts and the H pipeline on m (high priority), accumulations on q (low priority), tails on side streams; longest tail
    // (G2) first.  A sort that finishes on m releases its accumulation on q through ev_sort.
    hipStream_t m = c->s_main, q = c->s_acc;
    const DeviceTables *t = c->tables;
    const uint32_t k = c->cur_batch, ws = c->V + 1;             // proofs of this launch sequence; witness stride
    // a synchronous call (one proof, the caller waits) reduces its buckets with four lanes per point operation whatever the size:
    // 3.5x shorter tails for 4x the lanes (sync zk_prove at 2^18 3.98 -> 3.75 ms, at 2^20 13.2 -> 12.2 ms incl. the upload; pipelined
    // proofs of those sizes lose 6 % of throughput with it and keep one lane)
    if (phase != PHASE_H) c->alone_hint = c->device >= 0 && c->device < 64 && g_dev_inflight[c->device].load(std::memory_order_relaxed) == 0;
    const uint32_t tail_lanes = (c->latency_call || c->alone_hint) ? 4 : 0;
    auto release = [&]() -> int { if (q != m) { ZK_HIP(hipEventRecord(c->ev_sort, m)); ZK_HIP(hipStreamWaitEvent(q, c->ev_sort, 0)); } return ZK_OK; };
    // the H pipeline: on s_main behind the witness sorts, or -- split -- on its own stream beside them (it only needs the upload);
    // its launches are queued right after the first sort, ahead of the reductions' (the host enqueues ~5 us per launch)
    // Small proofs (domains up to 2^15, unbatched: fewer than 3 * 2^18 bucket entries per query) run the H pipeline beside the witness
    // sorts instead of behind them; it borrows a tail stream -- a sixth stream per context, even an idle one, changes how the
    // runtime maps streams to its hardware queues (created with the others it cost the pipelined 2^20 schedule 7 %, created on first
    // use it slowed the very proofs it was meant for by 15 %).  Which one is measured (tools/dev_sync_latency.py, bench.py):
    //  * a synchronous call (zk_prove, zk_prove_partial: the caller waits for this one proof) borrows the A-tail stream: the A tail
    //    is early and not critical, and at the end the L tail and the H tail run side by side -- Merkle-29 1.55 -> 1.23 ms, MiMC-11
    //    1.21 -> 1.10 ms, 2^14 1.46 -> 1.35 ms (the B-tail stream, the longest tail's, makes everything 30-50 % slower; 2^16: no gain);
    //  * queued proofs (zk_prove_submit, several contexts in flight) borrow the L-tail stream: Merkle-29 849 -> 949, MiMC-11
    //    1 083 -> 1 303 proofs/s with three contexts (the A-tail stream: no gain there; 2^16 and larger, and batches: -2 ... -7 %).
    const uint64_t entries = (uint64_t)c->mH.sh.max_entries() * k;
    // tuning aids (cached at context creation): ZK_H_STREAM=0 / 1 forces it, ZK_H_BORROW=a / l / b picks the stream
    const bool want_split = phase == PHASE_ALL && !c->serial && (c->env_h_stream >= 0 ? c->env_h_stream == 1 : entries < (3ull << 18));   // (a proof submitted in two phases keeps the H part on s_main)
    if (want_split && !c->h_stream_made) {
        ZK_HIP(hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
        ZK_HIP(hipEventCreateWithFlags(&c->ev_sort_h, hipEventDisableTiming));
        c->h_stream_made = true;
    }
    if (want_split) {
        const char which = c->env_h_borrow ? c->env_h_borrow : (c->latency_call ? 'a' : 'l');
        c->s_h = which == 'a' ? c->s_a : which == 'b' ? c->s_b : c->s_l;
    }
    const bool split_h = want_split && c->h_stream_made;
    hipStream_t hs = split_h ? c->s_h : m;
    auto h_pipeline = [&]() -> int {
        ZK_HIP(hipEventRecord(c->ev_h0, hs));
        if (!d_h) ZK_TRY(c->lag ? enqueue_compute_h4(c, hs) : enqueue_compute_h(c, hs));
        else {
            memset(c->h_tail, 0, 32);                           // the rank that computed h has checked its degree
            if (c->lag) ZK_TRY(enqueue_h_coefficients_to_coset(c, d_h, hs));
        }
        ZK_HIP(hipEventRecord(c->ev_h, hs));
        if (c->lag) ZK_TRY(c->mH.enqueue_sort(c->d_t, nullptr, c->m, d_h ? 0 : 1, hs, k, c->m));         // the m scalars p_j (canonical out of k_hl_product)
        else ZK_TRY(c->mH.enqueue_sort(d_h ? d_h : c->d_t + c->rH.lo, nullptr, c->rH.n(), 0, hs, k, c->m));   // tcc:510-518
        if (split_h) ZK_HIP(hipEventRecord(c->ev_sort_h, hs));
        return ZK_OK;
    };
    // Two other places for the H pipeline of ONE large synchronous proof were measured and are not taken (tools/dev_sync_latency.py,
    // 2^20 / 2^18): FIRST and alone, the accumulations released when it is done -- 11.97 / 3.94 ms against 11.09 / 3.76: beside the
    // accumulations it crawls (7.9 ms instead of 1.35 in the rocprofv3 timeline, profiles/r03_sync_timeline_2p20.txt) but its memory-bound
    // kernels do overlap with them; its launches queued right behind the B-query's instead of behind the L-query's (host order) -- no change.
    if (phase != PHASE_H) {
    if (split_h) { ZK_HIP(hipEventRecord(c->ev_up, m)); ZK_HIP(hipStreamWaitEvent(hs, c->ev_up, 0)); }
    if (t->share_A || t->share_B || t->share_L) {               // one sort of the witness digits of the window
        ZK_TRY(c->mW.enqueue_sort(c->d_w + t->win_lo, nullptr, t->win_n, 0, m, k, ws));
        ZK_TRY(release());
    }
    if (!t->share_B) { ZK_TRY(c->mB.enqueue_sort(c->d_w, c->dB_idx, c->rB.n(), 0, m, k, ws)); ZK_TRY(release()); }
    if (split_h) ZK_TRY(h_pipeline());
    ZK_HIP(hipEventRecord(c->ev_b0, q));
    ZK_TRY(c->mB.enqueue_reduce(t->share_B ? c->mW.view_for(t->offB, t->posB) : c->mB.view(), q, c->env_tails_on_acc ? q : c->s_b, c->env_b_tail_lanes ? (uint32_t)c->env_b_tail_lanes : tail_lanes));    // tcc:499-506
    ZK_HIP(hipEventRecord(c->ev_b1, c->s_b));
    if (zk) {
        // B = beta2 + Bt + s delta2 right behind the B-query's own tail (k_zk_blind_g2 needs nothing else)
        BlindG2Args g2{c->mB.partial_b, c->mB.sh.planes(), c->mB.sh.c, c->beta_g2, t->tD2, (const fe *)c->d_zk, (G2::XYZZ *)(c->d_zk + zk_g2_at), k};
        ZK_LAUNCH(k_zk_blind_g2, zk_div_up((uint64_t)k * BLIND_Q, BLIND_BLOCK), BLIND_BLOCK, c->s_b, g2);
        ZK_HIP(hipEventRecord(c->ev_z2, c->s_b));
        ZK_HIP(hipMemcpyAsync(c->h_zk + zk_g2_at, c->d_zk + zk_g2_at, BLIND_G2_BYTES * k, hipMemcpyDeviceToHost, c->s_b));
        // B1t: the G1 half of the B-query reads the B-query's sorted entries.  Its accumulation follows the B-query's on the
        // accumulation stream, so that it runs while the G2 tail does; its tail goes to the A-tail stream, ahead of the A-query's
        ZK_TRY(c->mB1.enqueue_accumulate(t->share_B ? c->mW.view_for(t->offB, t->posB) : c->mB.view(), q));
        ZK_TRY(c->mB1.enqueue_tail(c->env_tails_on_acc ? q : c->s_a, tail_lanes));
    }
    if (!t->share_A) { ZK_TRY(c->mA.enqueue_sort(c->d_w, c->dA_idx, c->rA.n(), 0, m, k, ws)); ZK_TRY(release()); }
    ZK_HIP(hipEventRecord(c->ev_a0, q));
    ZK_TRY(c->mA.enqueue_reduce(t->share_A ? c->mW.view_for(t->offA, t->posA) : c->mA.view(), q, c->env_tails_on_acc ? q : c->s_a, tail_lanes));    // tcc:488-495
    ZK_HIP(hipEventRecord(c->ev_a1, c->s_a));
    if (!t->share_L) { ZK_TRY(c->mL.enqueue_sort(c->d_w + c->l_first + c->rL.lo, nullptr, c->rL.n(), 0, m, k, ws)); ZK_TRY(release()); }
    // One synchronous proof below ~2^19 constraints is a latency chain: folded into the H-query's reduction the L-query's pieces double the
    // serial additions per bucket at the very end of the proof, while a tail of its own runs early, beside the H pipeline (same-box A/B,
    // tools/dev_sync_latency.py: 2^16 1.60 -> 1.65 ms, 2^18 3.38 -> 3.46 merged; 2^20 9.96 -> 9.94; pipelined 2^20: +2.8 % merged).  Sharded
    // contexts fold whenever they can (their device-side partial sums carry Lt = infinity).
    c->cur_merge = c->merge_hl && (c->cfg.shard_count > 1 || !c->latency_call || entries >= (1ull << 23));
    ZK_HIP(hipEventRecord(c->ev_l0, q));
    if (c->cur_merge) {                                          // tcc:522-530; its chunk pieces wait for the H-query's bucket reduction (tcc:540: C = Ht + Lt)
        ZK_TRY(c->mL.enqueue_accumulate(t->share_L ? c->mW.view_for(t->offL) : c->mL.view(), q));
        ZK_HIP(hipEventRecord(c->ev_l1, q));
    } else {
        ZK_TRY(c->mL.enqueue_reduce(t->share_L ? c->mW.view_for(t->offL) : c->mL.view(), q, c->env_tails_on_acc ? q : c->s_l, tail_lanes));
        ZK_HIP(hipEventRecord(c->ev_l1, c->s_l));
    }
    }
    if (phase == PHASE_WITNESS) return ZK_OK;                   // the H-query follows with zk_prove_submit_h
    if (!split_h) { ZK_TRY(h_pipeline()); ZK_TRY(release()); }
    else ZK_HIP(hipStreamWaitEvent(q, c->ev_sort_h, 0));
    ZK_TRY(c->mH.enqueue_accumulate(c->mH.view(), q));
    hipStream_t ts = hs;                                        // stream of the (merged) H tail
    if (c->env_tails_on_acc) ts = q;
    else if (c->cur_merge && !c->serial && c->env_hl_tail) ts = c->env_hl_tail == 'l' ? c->s_l : c->env_hl_tail == 'a' ? c->s_a : hs;
    ZK_TRY(c->mH.enqueue_tail(ts, tail_lanes, c->cur_merge ? &c->mL : nullptr));     // one bucket reduction for Ht + Lt
    ZK_HIP(hipEventRecord(c->ev_h1, ts));
    if (zk) {       // A and C from every G1 result: on the A-tail stream (behind the B1 and A tails), once the H and L tails are done
        hipStream_t bs = c->env_tails_on_acc ? q : c->s_a;
        ZK_HIP(hipStreamWaitEvent(bs, c->ev_h1, 0)); ZK_HIP(hipStreamWaitEvent(bs, c->ev_l1, 0)); ZK_HIP(hipStreamWaitEvent(bs, c->ev_zf, 0));
        BlindG1Args g1{c->mA.partial_b, c->mB1.partial_b, c->mH.partial_b, c->cur_merge ? nullptr : c->mL.partial_b,
                       c->mA.sh.planes(), c->mA.sh.c, c->mB1.sh.c, c->mH.sh.c, c->mL.sh.c, c->alpha_g1, c->beta_g1, (const G1::XYZZ *)(c->d_zk + zk_fix_at),
                       (const fe *)c->d_zk, (G1::XYZZ *)(c->d_zk + zk_g1_at), k};
        ZK_LAUNCH(k_zk_blind_g1, zk_div_up((uint64_t)k * BLIND_Q, BLIND_BLOCK), BLIND_BLOCK, bs, g1);
        ZK_HIP(hipEventRecord(c->ev_z1, bs));
        ZK_HIP(hipMemcpyAsync(c->h_zk + zk_g1_at, c->d_zk + zk_g1_at, BLIND_G1_BYTES * k, hipMemcpyDeviceToHost, bs));
    }
    return ZK_OK;
}

static int prove_collect_impl(zk_ctx *c, zk_partials *out, zk_timings *tm) {     // out == nullptr: the caller takes the device copy
    if (!c) return fail(ZK_ERR_ARG, "null argument");
    if (!c->in_flight) return fail(ZK_ERR_ARG, "no proof in flight on this context");
    if (c->awaiting_h) return fail(ZK_ERR_ARG, "the proof in flight has no H part yet (zk_prove_submit_h, or zk_prove_abort to drop it)");
    ZK_TRY(use_device(c->device));
    c->set_in_flight(false);
    ZK_HIP(hipStreamSynchronize(c->s_acc)); ZK_HIP(hipStreamSynchronize(c->s_a)); ZK_HIP(hipStreamSynchronize(c->s_b));
    ZK_HIP(hipStreamSynchronize(c->s_l)); ZK_HIP(hipStreamSynchronize(c->s_h)); ZK_HIP(hipStreamSynchronize(c->s_main));
    for (uint32_t p = 0; p < c->cur_batch; p++)
        if (!Fr::is_zero(c->h_tail[p])) return fail(ZK_ERR_DEGREE, "h[m-1] != 0: the witness does not satisfy the constraint system");
    double t0 = now_ms();
    if (out) for (uint32_t p = 0; p < c->cur_batch; p++) {      // out: cur_batch records
        store_xyzz(out[p].At, c->mA.finish(p)); store_xyzz(out[p].Bt, c->mB.finish(p));
        store_xyzz(out[p].Ht, c->mH.finish(p)); store_xyzz(out[p].Lt, c->mL.finish(p));
    } else if (c->tables->plog && !c->cur_zk) {                 // device copy of a sharded context with frugal tables: the planes are folded here, on the host
        std::vector<zk_partials> parts(c->cur_batch);
        for (uint32_t p = 0; p < c->cur_batch; p++) {
            store_xyzz(parts[p].At, c->mA.finish(p)); store_xyzz(parts[p].Bt, c->mB.finish(p));
            store_xyzz(parts[p].Ht, c->mH.finish(p)); store_xyzz(parts[p].Lt, c->mL.finish(p));
        }
        ZK_HIP(hipMemcpy(c->d_partials, parts.data(), sizeof(zk_partials) * c->cur_batch, hipMemcpyHostToDevice));
    }
    if (tm) {
        memset(tm, 0, sizeof(*tm));
        hipEventElapsedTime(&tm->h2d_witness, c->ev_start, c->ev_w);
        hipEventElapsedTime(&tm->compute_h, c->ev_h0, c->ev_h);
        hipEventElapsedTime(&tm->a_query, c->ev_a0, c->ev_a1);
        hipEventElapsedTime(&tm->b_query, c->ev_b0, c->ev_b1);
        hipEventElapsedTime(&tm->l_query, c->ev_l0, c->ev_l1);
        hipEventElapsedTime(&tm->h_query, c->ev_h, c->ev_h1);
        float ta = 0, tb = 0, tl = 0, th = 0;
        hipEventElapsedTime(&ta, c->ev_start, c->ev_a1); hipEventElapsedTime(&tb, c->ev_start, c->ev_b1);
        hipEventElapsedTime(&tl, c->ev_start, c->ev_l1); hipEventElapsedTime(&th, c->ev_start, c->ev_h1);
        tm->gpu_total = ta; if (tb > tm->gpu_total) tm->gpu_total = tb;
        if (tl > tm->gpu_total) tm->gpu_total = tl; if (th > tm->gpu_total) tm->gpu_total = th;
        if (c->cur_zk) {                                        // a zero-knowledge proof ends with its blinding kernels
            float z1 = 0, z2 = 0;
            hipEventElapsedTime(&z1, c->ev_start, c->ev_z1); hipEventElapsedTime(&z2, c->ev_start, c->ev_z2);
            if (z1 > tm->gpu_total) tm->gpu_total = z1; if (z2 > tm->gpu_total) tm->gpu_total = z2;
        }
        tm->host_finish = (float)(now_ms() - t0);
        tm->acc_a = c->mA.accumulate_ms(); tm->acc_b = c->mB.accumulate_ms();
        tm->acc_h = c->mH.accumulate_ms(); tm->acc_l = c->mL.accumulate_ms();
    }
    return ZK_OK;
}


static int prove_partial_impl(zk_ctx *c, const uint64_t *witness, int canonical, zk_partials *out, zk_timings *tm) {
    if (!out) return fail(ZK_ERR_ARG, "null argument");
    if (c) c->latency_call = true;                              // synchronous: one proof, the caller waits for it
    const int rc_submit = prove_submit_impl(c, witness, canonical);
    if (c) c->latency_call = false;
    ZK_TRY(rc_submit);
    return prove_collect_impl(c, out, tm);
}
// asynchronous form: enqueue a proof and return; collect later (lets two contexts keep the GPU full)
extern "C" int zk_prove_submit(zk_ctx *ctx, const uint64_t *witness, int canonical) try { return prove_submit_impl(ctx, witness, canonical); } ZK_GUARD
extern "C" int zk_prove_submit_resident(zk_ctx *ctx, const void *d_witness, int canonical) try { return prove_submit_impl(ctx, (const uint64_t *)d_witness, canonical, 1); } ZK_GUARD
// the witness lies in PINNED host memory ("witness already in pinned host memory"): the asynchronous H2D copy reads
// the caller's buffer itself -- no copy into the context's staging buffer --, so the buffer stays untouched until the proof is collected
extern "C" int zk_prove_submit_pinned(zk_ctx *ctx, const uint64_t *witness, int canonical) try { return prove_submit_impl(ctx, witness, canonical, 3); } ZK_GUARD
extern "C" int zk_prove_batch_submit_pinned(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical) try { return prove_submit_impl(ctx, witnesses, canonical, 3, k); } ZK_GUARD
extern "C" int zk_host_alloc(size_t bytes, void **out) try {
    if (!out) return fail(ZK_ERR_ARG, "null argument");
    ZK_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_host_free(void *p) try { if (p) ZK_HIP(hipHostFree(p)); return ZK_OK; } ZK_GUARD
extern "C" int zk_host_register(void *p, size_t bytes) try {
    if (!p || !bytes) return fail(ZK_ERR_ARG, "null argument");
    ZK_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_host_unregister(void *p) try { if (p) ZK_HIP(hipHostUnregister(p)); return ZK_OK; } ZK_GUARD
// ---- double-buffered upload: the NEXT witness (k of them, contiguous) goes to the device on a copy stream while a
// proof may still be in flight on this context; zk_prove_submit_staged then starts it with no upload on its critical path
static int prove_stage_impl(zk_ctx *c, const uint64_t *witnesses, uint32_t k, int canonical, bool pinned) {
    if (!c || !witnesses) return fail(ZK_ERR_ARG, "null argument");
    if (!k || k > c->max_batch) return fail(ZK_ERR_ARG, "batch size exceeds zk_config.max_batch of this context");
    if (c->staged_k) return fail(ZK_ERR_ARG, "a witness is already staged on this context (submit it first)");
    ZK_TRY(use_device(c->device));
    const size_t cap = 32 * (size_t)(c->V + 1) * c->max_batch, n = 32 * (size_t)(c->V + 1) * k;
    if (!c->d_w2) {
        ZK_HIP(hipMalloc(&c->d_w2, cap));
        ZK_HIP(hipHostMalloc(&c->h_w2, cap, hipHostMallocDefault));
        int lo = 0, hi = 0;
        ZK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        c->stream_prio[ROLE_COPY] = (lo + hi) / 2;
        ZK_TRY(stream_take(&c->s_copy, c->device, ROLE_COPY, c->stream_prio[ROLE_COPY]));
        ZK_HIP(hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming));
    }
    if (!pinned) {
        ZK_HIP(hipStreamSynchronize(c->s_copy));                // (the previous staged copy out of h_w2 has long finished; cheap)
        memcpy(c->h_w2, witnesses, n);
    }
    ZK_HIP(hipMemcpyAsync(c->d_w2, pinned ? (const void *)witnesses : (const void *)c->h_w2, n, hipMemcpyHostToDevice, c->s_copy));
    ZK_HIP(hipEventRecord(c->ev_staged, c->s_copy));
    c->staged_k = k; c->staged_canonical = canonical;
    return ZK_OK;
}
extern "C" int zk_prove_stage(zk_ctx *c, const uint64_t *witnesses, uint32_t k, int canonical) try { return prove_stage_impl(c, witnesses, k, canonical, false); } ZK_GUARD
// the same from PINNED host memory: the copy stream reads the caller's buffer where it lies (untouched until that proof is collected)
extern "C" int zk_prove_stage_pinned(zk_ctx *c, const uint64_t *witnesses, uint32_t k, int canonical) try { return prove_stage_impl(c, witnesses, k, canonical, true); } ZK_GUARD
extern "C" int zk_prove_submit_staged(zk_ctx *c) try {
    if (!c) return fail(ZK_ERR_ARG, "null argument");
    if (!c->staged_k) return fail(ZK_ERR_ARG, "no staged witness on this context (zk_prove_stage first)");
    if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is already in flight on this context (collect it first)");
    std::swap(c->d_w, c->d_w2);                                 // the collected proof no longer reads the old buffer
    const uint32_t k = c->staged_k;
    const int rc = prove_submit_impl(c, (const uint64_t *)c->d_w, c->staged_canonical, 2, k);
    if (rc != ZK_OK) { std::swap(c->d_w, c->d_w2); return rc; }    // nothing is in flight (the failed submit was drained): the staged witness stays staged and can be submitted again
    c->staged_k = 0;
    return ZK_OK;
} ZK_GUARD
// ---- SURVEY 8(e) option 2: the transform chains of the witness map on different ranks (ethsnarks_amd/sharded.py drives it)
extern "C" int zk_chain_submit(zk_ctx *c, const uint64_t *witness, int canonical, int which) try {
    if (!c || which < 0 || which > 2) return fail(ZK_ERR_ARG, "bad argument");
    ZK_TRY(use_device(c->device));
    if (c->in_flight && c->awaiting_h) {                        // the witness of the deferred proof is already on the device (same stream: ordered)
        if (c->cur_batch != 1) return fail(ZK_ERR_ARG, "zk_chain_submit: the deferred proof is a batch");
        return enqueue_chain(c, which);
    }
    if (!witness) return fail(ZK_ERR_ARG, "null argument");
    if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is in flight on this context (collect it first)");
    c->cur_batch = 1;
    ZK_TRY(upload_witness(c, witness, canonical));
    return enqueue_chain(c, which);
} ZK_GUARD
extern "C" const void *zk_chain_device(const zk_ctx *c, int which) {
    if (!c || which < 0 || which > 2) return nullptr;
    return which == 2 ? c->d_t + 2 * (size_t)c->m : c->d_a + (size_t)which * c->m;       // A, B: coset evaluations; C: coefficients / Z(g)
}
extern "C" int zk_h_from_chains_submit(zk_ctx *c, const void *dA, const void *dB, const void *dC) try {
    if (!c || !dA || !dB || !dC) return fail(ZK_ERR_ARG, "null argument");
    if (c->in_flight && !c->awaiting_h) return fail(ZK_ERR_ARG, "a proof is in flight on this context (collect it first)");
    ZK_TRY(use_device(c->device));
    return enqueue_h_from_chains(c, (const fe *)dA, (const fe *)dB, (const fe *)dC);
} ZK_GUARD
extern "C" const void *zk_h_device(const zk_ctx *c) { return c ? c->d_t : nullptr; }
// waits for the chain / h work queued so far; after zk_h_from_chains_submit it also checks the degree of h
extern "C" int zk_chain_wait(zk_ctx *c, int check_degree) try {
    if (!c) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(c->device));
    ZK_HIP(hipStreamSynchronize(c->s_main));
    if (check_degree && !Fr::is_zero(c->h_tail[0])) return fail(ZK_ERR_DEGREE, "h[m-1] != 0: the witness does not satisfy the constraint system");
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_prove_submit_with_h(zk_ctx *c, const uint64_t *witness, int canonical, const void *d_h) try {
    if (!d_h) return fail(ZK_ERR_ARG, "null argument");
    return prove_submit_impl(c, witness, canonical, 0, 1, (const fe *)d_h);
} ZK_GUARD
// the same proof in two steps, so that the ranks of option 2 start their witness sorts and A-, B-, L-query accumulations BEFORE H
// exists: zk_prove_submit_defer_h queues everything that needs only the witness; zk_chain_submit / zk_h_from_chains_submit may follow
// on this context (witness = NULL: the deferred proof's witness is used); zk_prove_submit_h queues the H-query; collect as usual.
// zk_prove_abort drops a proof that will not get its H part (another rank found the witness unsatisfying): drains, frees the context.
extern "C" int zk_prove_submit_defer_h(zk_ctx *c, const uint64_t *witness, int canonical) try { return prove_submit_impl(c, witness, canonical, 0, 1, nullptr, PHASE_WITNESS); } ZK_GUARD
extern "C" int zk_prove_submit_h(zk_ctx *c, const void *d_h) try { return prove_submit_impl(c, nullptr, 0, 0, 1, (const fe *)d_h, PHASE_H); } ZK_GUARD
extern "C" int zk_prove_abort(zk_ctx *c) try {
    if (!c) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(c->device));
    drain(c);
    c->set_in_flight(false); c->awaiting_h = false;
    if (c->cur_zk) zk_clear_rs(c);
    return ZK_OK;
} ZK_GUARD

// ---- several proofs of the circuit through ONE launch sequence: k witnesses, contiguous, k <= zk_config.max_batch
extern "C" int zk_prove_batch_submit(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical) try { return prove_submit_impl(ctx, witnesses, canonical, 0, k); } ZK_GUARD
extern "C" int zk_prove_batch_submit_resident(zk_ctx *ctx, const void *d_witnesses, uint32_t k, int canonical) try { return prove_submit_impl(ctx, (const uint64_t *)d_witnesses, canonical, 1, k); } ZK_GUARD
extern "C" int zk_prove_batch_collect(zk_ctx *ctx, zk_partials *out, uint32_t k, zk_timings *t) try {
    if (!ctx || !out) return fail(ZK_ERR_ARG, "null argument");
    if (ctx && ctx->in_flight && ctx->cur_zk) return fail(ZK_ERR_ARG, "a zero-knowledge proof is in flight: collect it with zk_prove_zk_batch_collect");
    if (ctx->in_flight && k != ctx->cur_batch) return fail(ZK_ERR_ARG, "collect: k differs from the submitted batch size");
    return prove_collect_impl(ctx, out, t);
} ZK_GUARD
extern "C" int zk_prove_batch(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, zk_proof *out) try {
    if (!ctx || !out) return fail(ZK_ERR_ARG, "null argument");
    if (ctx->cfg.shard_count > 1) return fail(ZK_ERR_ARG, "sharded context: use zk_prove_batch_submit / _collect + zk_prove_combine per proof");
    ZK_TRY(prove_submit_impl(ctx, witnesses, canonical, 0, k));
    std::vector<zk_partials> parts(k);
    ZK_TRY(prove_collect_impl(ctx, parts.data(), nullptr));
    for (uint32_t p = 0; p < k; p++) ZK_TRY(zk_prove_combine(ctx, &parts[p], 1, &out[p]));
    return ZK_OK;
} ZK_GUARD
// what the context chose: {window bits, windows, buckets} of the A-, B-, H-, L-query MSMs, then whether the witness sort is shared
extern "C" int zk_ctx_info(const zk_ctx *c, uint32_t info[16]) try {
    if (!c || !info) return fail(ZK_ERR_ARG, "null argument");
    const MsmShape *sh[4] = {&c->mA.sh, &c->mB.sh, &c->mH.sh, &c->mL.sh};
    for (int i = 0; i < 4; i++) { info[3 * i] = sh[i]->c; info[3 * i + 1] = sh[i]->W; info[3 * i + 2] = sh[i]->nb; }
    info[12] = c->tables->share_A; info[13] = c->tables->share_B; info[14] = c->tables->share_L; info[15] = c->m;
    return ZK_OK;
} ZK_GUARD
// the window-multiple tables of the context: {bytes they take, bytes all W windows would take, planes S (1 = every window is tabulated), table rows of the B-query}
extern "C" int zk_ctx_table_info(const zk_ctx *c, uint64_t info[4]) try {
    if (!c || !info) return fail(ZK_ERR_ARG, "null argument");
    info[0] = c->tables->table_bytes; info[1] = c->tables->full_table_bytes; info[2] = 1ull << c->tables->plog; info[3] = c->mB.sh.rows();
    return ZK_OK;
} ZK_GUARD
// the H-query in coset-Lagrange bases: {1 if this context proves with four transforms, microseconds the transform of the bases took when the
// tables were built (once per key and circuit), 0, 0}
extern "C" int zk_ctx_hlagrange_info(const zk_ctx *c, uint64_t info[4]) try {
    if (!c || !info) return fail(ZK_ERR_ARG, "null argument");
    info[0] = c->lag ? 1 : 0; info[1] = (uint64_t)(c->tables->lag_ms * 1000.0); info[2] = 0; info[3] = 0;
    return ZK_OK;
} ZK_GUARD
// test entry points of the per-key transform (hlagrange.hpp): points are affine, 8 x u64 each, Montgomery Fq, (0, 0) = the point at infinity
extern "C" int zk_hl_probe_dft(const uint64_t *points, uint32_t n, uint32_t logm, int coset, int device, uint64_t *out) try {
    if (!points || !out || logm > 20 || n > (1u << logm)) return fail(ZK_ERR_ARG, "bad argument");
    ZK_TRY(use_device(device));
    const uint32_t m = 1u << logm;
    DevScratch s;
    G1::Affine *d_out = nullptr;
    ZK_TRY(s.get(&d_out, m));
    ZK_TRY(hl_group_dft((const G1::Affine *)points, n, logm, coset != 0, d_out));
    ZK_HIP(hipMemcpy(out, d_out, sizeof(G1::Affine) * (size_t)m, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_hl_probe_columns(const zk_csr *Cm, uint32_t nIn, uint32_t V, const uint64_t *lambda, uint32_t m, const uint64_t *l_bases, int device, uint64_t *out) try {
    if (!Cm || !lambda || !out || nIn > V || (!l_bases && V != nIn) || Cm->n_rows > m) return fail(ZK_ERR_ARG, "bad argument");
    ZK_TRY(use_device(device));
    DevScratch s;
    G1::Affine *d_lam = nullptr, *d_lk = nullptr;
    ZK_TRY(s.put(&d_lam, (const G1::Affine *)lambda, m));
    ZK_TRY(s.get(&d_lk, (size_t)V + 1));
    ZK_TRY(hl_column_bases(d_lam, (const G1::Affine *)l_bases, Cm, nIn, V, d_lk));
    ZK_HIP(hipMemcpy(out, d_lk, sizeof(G1::Affine) * ((size_t)V + 1), hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_prove_collect(zk_ctx *ctx, zk_partials *out, zk_timings *t) try {
    if (!ctx || !out) return fail(ZK_ERR_ARG, "null argument");
    if (ctx && ctx->in_flight && ctx->cur_zk) return fail(ZK_ERR_ARG, "a zero-knowledge proof is in flight: collect it with zk_prove_zk_batch_collect");
    if (ctx->in_flight && ctx->cur_batch != 1) return fail(ZK_ERR_ARG, "a batch is in flight: use zk_prove_batch_collect");
    return prove_collect_impl(ctx, out, t);
} ZK_GUARD
// device-side exchange of sharded provers: the partial sums stay in a 640-byte device buffer of the context (zk_partials layout,
// loose Montgomery values), ready for an RCCL all-gather; zk_prove_combine_device takes the gathered device buffer
extern "C" const void *zk_ctx_partials_device(const zk_ctx *ctx) { return ctx ? ctx->d_partials : nullptr; }
extern "C" int zk_prove_collect_device(zk_ctx *ctx, zk_timings *t) try {
    if (ctx && ctx->in_flight && ctx->cur_zk) return fail(ZK_ERR_ARG, "a zero-knowledge proof is in flight: collect it with zk_prove_zk_batch_collect");
    if (ctx && ctx->cfg.shard_count <= 1) return fail(ZK_ERR_ARG, "zk_prove_collect_device: only sharded contexts keep a device copy of their partial sums");
    return prove_collect_impl(ctx, nullptr, t);
} ZK_GUARD

template <class F> static void canon4(uint64_t dst[4], const fe &mont) { fe c = F::from_mont(mont); memcpy(dst, c.l, 32); }
static void put_g1(const G1::XYZZ &p, uint64_t x[4], uint64_t y[4], uint32_t *inf) {
    G1::Affine a = G1::to_affine(p);
    if (G1::is_inf(a)) { memset(x, 0, 32); memset(y, 0, 32); y[0] = 1; *inf = 1; return; }   // libff affine image of zero: (0, 1)
    canon4<Fq>(x, a.x); canon4<Fq>(y, a.y); *inf = 0;
}
static void put_g2(const G2::XYZZ &p, uint64_t xc0[4], uint64_t xc1[4], uint64_t yc0[4], uint64_t yc1[4], uint32_t *inf) {
    G2::Affine a = G2::to_affine(p);
    if (G2::is_inf(a)) { memset(xc0, 0, 32); memset(xc1, 0, 32); memset(yc0, 0, 32); memset(yc1, 0, 32); yc0[0] = 1; *inf = 1; return; }
    canon4<Fq>(xc0, a.x.c0); canon4<Fq>(xc1, a.x.c1); canon4<Fq>(yc0, a.y.c0); canon4<Fq>(yc1, a.y.c1); *inf = 0;
}

// "Compute the proof" tail, tcc:533-546: A = alpha + At, B = beta + Bt, C = Ht + Lt; partials folded in rank order
extern "C" int zk_prove_combine(const zk_ctx *c, const zk_partials *parts, uint32_t count, zk_proof *out) try {
    if (!c || !parts || !count || !out) return fail(ZK_ERR_ARG, "null argument");
    G1::XYZZ At = G1::infinity(), Ht = G1::infinity(), Lt = G1::infinity(); G2::XYZZ Bt = G2::infinity();
    for (uint32_t i = 0; i < count; i++) {
        G1::XYZZ a, h, l; G2::XYZZ b;
        memcpy(&a, parts[i].At, sizeof(a)); memcpy(&b, parts[i].Bt, sizeof(b));
        memcpy(&h, parts[i].Ht, sizeof(h)); memcpy(&l, parts[i].Lt, sizeof(l));
        At = G1::add(At, a); Bt = G2::add(Bt, b); Ht = G1::add(Ht, h); Lt = G1::add(Lt, l);
    }
    G1::XYZZ gA = G1::madd(At, c->alpha_g1);
    G2::XYZZ gB = G2::madd(Bt, c->beta_g2);
    G1::XYZZ gC = G1::add(Ht, Lt);
    memset(out, 0, sizeof(*out));
    put_g1(gA, out->a_x, out->a_y, &out->a_inf);
    put_g2(gB, out->b_x_c0, out->b_x_c1, out->b_y_c0, out->b_y_c1, &out->b_inf);
    put_g1(gC, out->c_x, out->c_y, &out->c_inf);
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_prove_combine_device(const zk_ctx *c, const void *d_parts, uint32_t count, zk_proof *out) try {
    if (!c || !d_parts || !count || !out) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(c->device));
    std::vector<zk_partials> parts(count);
    ZK_HIP(hipMemcpy(parts.data(), d_parts, sizeof(zk_partials) * (size_t)count, hipMemcpyDeviceToHost));
    for (auto &p : parts) {                                  // device values are loose ([0, 2p)): normalise once
        G1::XYZZ a, h, l; G2::XYZZ b;
        memcpy(&a, p.At, sizeof(a)); memcpy(&b, p.Bt, sizeof(b)); memcpy(&h, p.Ht, sizeof(h)); memcpy(&l, p.Lt, sizeof(l));
        store_xyzz(p.At, G1::canon(a)); store_xyzz(p.Bt, G2::canon(b)); store_xyzz(p.Ht, G1::canon(h)); store_xyzz(p.Lt, G1::canon(l));
    }
    return zk_prove_combine(c, parts.data(), count, out);
} ZK_GUARD

extern "C" int zk_prove_partial(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_partials *out) try {
    return prove_partial_impl(ctx, witness, canonical, out, nullptr);
} ZK_GUARD
extern "C" int zk_prove_partial_timed(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_partials *out, zk_timings *t) try {
    return prove_partial_impl(ctx, witness, canonical, out, t);
} ZK_GUARD
extern "C" int zk_prove_timed(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_proof *out, zk_timings *t) try {
    if (!ctx || !out) return fail(ZK_ERR_ARG, "null argument");
    if (ctx->cfg.shard_count > 1) return fail(ZK_ERR_ARG, "sharded context: use zk_prove_partial + zk_prove_combine");
    zk_partials p;
    ZK_TRY(prove_partial_impl(ctx, witness, canonical, &p, t));
    double t0 = now_ms();
    ZK_TRY(zk_prove_combine(ctx, &p, 1, out));
    if (t) t->host_finish += (float)(now_ms() - t0);
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_prove(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_proof *out) try {
    return zk_prove_timed(ctx, witness, canonical, out, nullptr);
} ZK_GUARD

// ---- zero-knowledge proofs (libsnark's r1cs_gg_ppzksnark_prover): A + r delta1, B + s delta2, C + s A + r B1 - r s delta1, blinded
// on the device (blind.hpp).  Contexts of a full key only (tables->zk), unsharded; r, s per proof from the caller or from getrandom(2).
static bool fr_canonical(const uint64_t v[4]) {
    for (int i = 3; i >= 0; i--) {
        const uint64_t p = (uint64_t)FrParams::p(2 * i) | ((uint64_t)FrParams::p(2 * i + 1) << 32);
        if (v[i] != p) return v[i] < p;
    }
    return false;                                               // v == r
}
// one uniform scalar: 64 bytes of the operating system's CSPRNG reduced mod r (bias below 2^-250)
static int fr_draw(fe &out) {
    uint8_t buf[64];
    for (size_t got = 0; got < sizeof(buf);) {
        const ssize_t n = getrandom(buf + got, sizeof(buf) - got, 0);
        if (n < 0) { if (errno == EINTR) continue; return fail(ZK_ERR_INTERNAL, "getrandom(2) failed: no randomness for r, s"); }
        got += (size_t)n;
    }
    fe lo, hi, r2;
    memcpy(lo.l, buf, 32); memcpy(hi.l, buf + 32, 32);
    for (int i = 0; i < 8; i++) r2.l[i] = FrParams::r2(i);
    const fe a = Fr::mul(hi, r2);                               // hi R^2 / R = hi 2^256 mod r (any hi < 2^256)
    const fe b = Fr::from_mont(Fr::mul(lo, r2));                // lo mod r
    out = Fr::canon(Fr::add(a, b));
    volatile uint8_t *v = buf; for (size_t i = 0; i < sizeof(buf); i++) v[i] = 0;
    return ZK_OK;
}
static void zk_clear_rs(zk_ctx *c) {                           // the host and device copies of r, s of the proof that was collected or dropped
    volatile uint8_t *v = c->h_zk;
    for (size_t i = 0; i < BLIND_RS_BYTES * c->max_batch; i++) v[i] = 0;
    (void)hipMemset(c->d_zk, 0, BLIND_RS_BYTES * c->max_batch);
    c->cur_zk = false;
}
static int prove_zk_submit_impl(zk_ctx *c, const uint64_t *witness, int canonical, int resident, uint32_t k, const uint64_t *rs_canon) {
    if (!c || !witness) return fail(ZK_ERR_ARG, "null argument");
    if (c->cfg.shard_count > 1) return fail(ZK_ERR_ARG, "zero-knowledge proofs need an unsharded context (shard_count <= 1)");
    if (!c->tables->zk) return fail(ZK_ERR_ARG, "zero-knowledge proofs need a context created from a full proving key (zk_pk_load_raw_full / zk_keygen_full)");
    if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is already in flight on this context (collect it first)");
    if (!k || k > c->max_batch) return fail(ZK_ERR_ARG, "batch size exceeds zk_config.max_batch of this context");
    fe *rs = (fe *)c->h_zk;
    for (uint32_t p = 0; p < 2 * k; p++) {
        if (!rs_canon) { const int rc = fr_draw(rs[p]); if (rc != ZK_OK) { zk_clear_rs(c); return rc; } continue; }
        if (!fr_canonical(rs_canon + 4 * (size_t)p)) { zk_clear_rs(c); return fail(ZK_ERR_ARG, "r and s must be canonical scalars below the Fr modulus"); }
        memcpy(rs[p].l, rs_canon + 4 * (size_t)p, 32);
    }
    c->cur_zk = true;
    const int rc = prove_submit_impl(c, witness, canonical, resident, k);
    if (rc != ZK_OK) zk_clear_rs(c);
    return rc;
}
static int prove_zk_collect_impl(zk_ctx *c, zk_proof *out, uint32_t k, zk_timings *tm) {
    if (!c || !out) return fail(ZK_ERR_ARG, "null argument");
    if (c->in_flight && !c->cur_zk) return fail(ZK_ERR_ARG, "the proof in flight is not a zero-knowledge proof: collect it with zk_prove_collect / zk_prove_batch_collect");
    if (c->in_flight && k != c->cur_batch) return fail(ZK_ERR_ARG, "collect: k differs from the submitted batch size");
    const int rc = prove_collect_impl(c, nullptr, tm);          // (waits for every stream of the context)
    if (!c->cur_zk) return rc;                                  // nothing was in flight
    zk_clear_rs(c);
    ZK_TRY(rc);
    const double t0 = now_ms();
    const G1::XYZZ *g1 = (const G1::XYZZ *)(c->h_zk + BLIND_RS_BYTES * c->max_batch);
    const G2::XYZZ *g2 = (const G2::XYZZ *)(c->h_zk + (BLIND_RS_BYTES + BLIND_G1_BYTES) * c->max_batch);
    for (uint32_t p = 0; p < k; p++) {
        memset(&out[p], 0, sizeof(out[p]));
        put_g1(g1[2 * p], out[p].a_x, out[p].a_y, &out[p].a_inf);
        put_g2(g2[p], out[p].b_x_c0, out[p].b_x_c1, out[p].b_y_c0, out[p].b_y_c1, &out[p].b_inf);
        put_g1(g1[2 * p + 1], out[p].c_x, out[p].c_y, &out[p].c_inf);
    }
    if (tm) tm->host_finish += (float)(now_ms() - t0);
    return ZK_OK;
}
extern "C" int zk_prove_zk_batch_submit(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, const uint64_t *rs_canon) try {
    return prove_zk_submit_impl(ctx, witnesses, canonical, 0, k, rs_canon);
} ZK_GUARD
extern "C" int zk_prove_zk_batch_submit_resident(zk_ctx *ctx, const void *d_witnesses, uint32_t k, int canonical, const uint64_t *rs_canon) try {
    return prove_zk_submit_impl(ctx, (const uint64_t *)d_witnesses, canonical, 1, k, rs_canon);
} ZK_GUARD
extern "C" int zk_prove_zk_batch_collect(zk_ctx *ctx, zk_proof *out, uint32_t k, zk_timings *t) try {
    return prove_zk_collect_impl(ctx, out, k, t);
} ZK_GUARD
extern "C" int zk_prove_zk_batch(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, const uint64_t *rs_canon, zk_proof *out) try {
    if (!ctx || !out) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(prove_zk_submit_impl(ctx, witnesses, canonical, 0, k, rs_canon));
    return prove_zk_collect_impl(ctx, out, k, nullptr);
} ZK_GUARD
extern "C" int zk_prove_zk(zk_ctx *ctx, const uint64_t *witness, int canonical, const uint64_t *rs_canon, zk_proof *out) try {
    if (!ctx || !out) return fail(ZK_ERR_ARG, "null argument");
    ctx->latency_call = true;                                   // synchronous: one proof, the caller waits for it
    const int rc = prove_zk_submit_impl(ctx, witness, canonical, 0, 1, rs_canon);
    ctx->latency_call = false;
    ZK_TRY(rc);
    return prove_zk_collect_impl(ctx, out, 1, nullptr);
} ZK_GUARD


// ================================================================ key generation
// r1cs_gg_ppzksnark_zok_generator (tcc:277-449) with r1cs_to_qap_instance_map_with_evaluation
//  and the zk -> nozk conversion of hpp:209-233.
extern "C" void zk_vk_free(zk_vk *vk) try { delete vk; } ZK_GUARD_VOID

namespace {
// standard alt_bn128 G2 generator, canonical 32-bit limbs: x.c0, x.c1, y.c0, y.c1
const uint32_t G2_GEN_CANON[4][8] = {
    {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
    {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
    {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
    {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};
fe fq_from_canon32(const uint32_t v[8]) { fe t; for (int i = 0; i < 8; i++) t.l[i] = v[i]; return Fq::to_mont(t); }

void fr_batch_inverse(std::vector<fe> &a) {          // Montgomery's trick; zeros stay zero
    std::vector<fe> pre(a.size());
    fe acc = Fr::one();
    for (size_t i = 0; i < a.size(); i++) { pre[i] = acc; if (!Fr::is_zero(a[i])) acc = Fr::mul(acc, a[i]); }
    acc = Fr::inv(acc);
    for (size_t i = a.size(); i-- > 0;) {
        if (Fr::is_zero(a[i])) continue;
        fe t = Fr::mul(acc, pre[i]); acc = Fr::mul(acc, a[i]); a[i] = t;
    }
}
template <class C>
int batch_mul_host(const typename C::Affine &base, const std::vector<fe> &scalars, std::vector<typename C::Affine> &out) {
    out.resize(scalars.size());
    if (scalars.empty()) return ZK_OK;
    fe *d_s = nullptr; typename C::Affine *d_o = nullptr;
    int rc = dev_upload(&d_s, scalars.data(), scalars.size());
    if (rc == ZK_OK && hipMalloc(&d_o, sizeof(typename C::Affine) * scalars.size()) != hipSuccess) rc = ZK_ERR_NOMEM;
    if (rc == ZK_OK) rc = batch_mul_base<C>(base, d_s, (uint32_t)scalars.size(), d_o, nullptr);
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "batch_mul_base kernel failed");
    if (rc == ZK_OK && hipMemcpy(out.data(), d_o, sizeof(typename C::Affine) * scalars.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_ERR_HIP;
    if (d_s) hipFree(d_s);
    if (d_o) hipFree(d_o);
    return rc;
}
}  // namespace

// full: the key keeps the G1 half of the B-query as well (b1_val[i] = Bt_i G1, the knowledge commitments of tcc:371-380)
static int keygen_impl(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t nIn, uint32_t V,
                       const uint64_t toxic_canon[20], int device, zk_pk **pk_out, zk_vk **vk_out, bool full) {
    if (!A || !B || !C || !toxic_canon || !pk_out || !vk_out) return fail(ZK_ERR_ARG, "null argument");
    if (A->n_rows != nC || B->n_rows != nC || C->n_rows != nC || nIn > V) return fail(ZK_ERR_ARG, "inconsistent constraint system");
    if ((uint64_t)nC + nIn + 1 > (1ull << 28)) return fail(ZK_ERR_ARG, "domain exceeds 2^28");
    ZK_TRY(use_device(device));
    const uint32_t m = zk_domain_size(nC, nIn);
    uint32_t logm = 0; while ((1u << logm) < m) logm++;
    fe tox[5];
    for (int i = 0; i < 5; i++) { fe c; memcpy(c.l, toxic_canon + 4 * i, 32); tox[i] = Fr::to_mont(c); }
    const fe t = tox[0], alpha = tox[1], beta = tox[2], gamma = tox[3], delta = tox[4];
    if (Fr::is_zero(gamma) || Fr::is_zero(delta)) return fail(ZK_ERR_ARG, "gamma and delta must be invertible");
    // Lagrange basis at t: u_i = omega^i (t^m - 1) / (m (t - omega^i)); indicator vector if t is in the domain
    const fe w = fr_domain_root(logm), Zt = Fr::sub(Fr::pow_u64(t, m), Fr::one()), mfe = Fr::from_u64(m);
    std::vector<fe> u(m), den(m);
    fe wi = Fr::one();
    for (uint32_t i = 0; i < m; i++) {
        fe d = Fr::sub(t, wi);
        den[i] = Fr::mul(d, mfe);
        u[i] = Fr::is_zero(d) ? Fr::one() : Fr::mul(wi, Zt);
        if (Fr::is_zero(d)) den[i] = Fr::one();
        wi = Fr::mul(wi, w);
    }
    fr_batch_inverse(den);
    for (uint32_t i = 0; i < m; i++) u[i] = Fr::mul(u[i], den[i]);
    std::vector<fe> At(V + 1, Fr::zero()), Bt(V + 1, Fr::zero()), Ct(V + 1, Fr::zero());
    for (uint32_t i = 0; i <= nIn; i++) At[i] = u[nC + i];
    const zk_csr *Ms[3] = {A, B, C}; std::vector<fe> *Ts[3] = {&At, &Bt, &Ct};
    for (int q = 0; q < 3; q++) {
        const zk_csr *M = Ms[q];
        if (M->row_ptr[0] != 0) return fail(ZK_ERR_ARG, "CSR row_ptr[0] != 0");
        for (uint32_t j = 0; j < nC; j++)
            for (uint32_t k = M->row_ptr[j]; k < M->row_ptr[j + 1]; k++) {
                if (M->col[k] > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables");
                fe cf; memcpy(cf.l, M->coeff + 4 * (size_t)k, 32);
                fe p = fr_is_one(cf) ? u[j] : Fr::mul(u[j], cf);
                fe &dst = (*Ts[q])[M->col[k]];
                dst = Fr::add(dst, p);
            }
    }
    const fe gi = Fr::inv(gamma), di = Fr::inv(delta);
    // G1 scalars: [alpha, beta, delta | gammaABC (nIn+1) | A (non-zero) | H (m-1) | L (V-nIn)]
    std::vector<fe> s1, s2;
    std::unique_ptr<zk_pk> pk(new zk_pk()); std::unique_ptr<zk_vk> vk(new zk_vk());
    pk->a_domain = V + 1; pk->b_domain = V + 1;
    s1.push_back(alpha); s1.push_back(beta); s1.push_back(delta);
    s2.push_back(beta); s2.push_back(gamma); s2.push_back(delta);
    std::vector<fe> abc(V + 1);
    for (uint32_t i = 0; i <= V; i++) {                      // (beta At + alpha Bt + Ct) / {gamma | delta}, tcc:326-342
        fe v = Fr::add(Fr::add(Fr::mul(beta, At[i]), Fr::mul(alpha, Bt[i])), Ct[i]);
        abc[i] = Fr::mul(v, i <= nIn ? gi : di);
    }
    for (uint32_t i = 0; i <= nIn; i++) s1.push_back(abc[i]);
    for (uint32_t i = 0; i <= V; i++) if (!Fr::is_zero(At[i])) { pk->a_idx.push_back(i); s1.push_back(At[i]); }   // hpp:216-224
    for (uint32_t i = 0; i <= V; i++) if (!Fr::is_zero(Bt[i])) { pk->b_idx.push_back(i); s2.push_back(Bt[i]); }   // hpp:225-230
    {
        fe zd = Fr::mul(Zt, di), tj = Fr::one();               // H_j = t^j Zt / delta, j < m-1 (tcc:350,400)
        for (uint32_t j = 0; j + 1 < m; j++) { s1.push_back(Fr::mul(tj, zd)); tj = Fr::mul(tj, t); }
    }
    for (uint32_t i = nIn + 1; i <= V; i++) s1.push_back(abc[i]);
    if (full) for (uint32_t i = 0; i <= V; i++) if (!Fr::is_zero(Bt[i])) s1.push_back(Bt[i]);   // the B-query's G1 half, after L
    G1::Affine g1; g1.x = Fq::from_u64(1); g1.y = Fq::from_u64(2);
    G2::Affine g2;
    g2.x.c0 = fq_from_canon32(G2_GEN_CANON[0]); g2.x.c1 = fq_from_canon32(G2_GEN_CANON[1]);
    g2.y.c0 = fq_from_canon32(G2_GEN_CANON[2]); g2.y.c1 = fq_from_canon32(G2_GEN_CANON[3]);
    std::vector<G1::Affine> o1; std::vector<G2::Affine> o2;
    int rc = batch_mul_host<G1>(g1, s1, o1);
    if (rc == ZK_OK) rc = batch_mul_host<G2>(g2, s2, o2);
    if (rc != ZK_OK) return rc;
    size_t k = 0;
    pk->alpha_g1 = o1[k++]; pk->beta_g1 = o1[k++]; pk->delta_g1 = o1[k++];
    vk->gamma_abc.assign(o1.begin() + k, o1.begin() + k + nIn + 1); k += nIn + 1;
    pk->a_val.assign(o1.begin() + k, o1.begin() + k + pk->a_idx.size()); k += pk->a_idx.size();
    pk->H.assign(o1.begin() + k, o1.begin() + k + (m - 1)); k += m - 1;
    pk->L.assign(o1.begin() + k, o1.begin() + k + (V - nIn)); k += V - nIn;
    if (full) { pk->b1_val.assign(o1.begin() + k, o1.end()); pk->full = true; }
    pk->beta_g2 = o2[0]; pk->delta_g2 = o2[2];
    pk->b_val.assign(o2.begin() + 3, o2.end());
    vk->alpha_g1 = pk->alpha_g1; vk->beta_g2 = o2[0]; vk->gamma_g2 = o2[1]; vk->delta_g2 = o2[2];
    *pk_out = pk.release(); *vk_out = vk.release();
    return ZK_OK;
}
extern "C" int zk_keygen(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t nIn, uint32_t V,
                         const uint64_t toxic_canon[20], int device, zk_pk **pk_out, zk_vk **vk_out) try {
    return keygen_impl(A, B, C, nC, nIn, V, toxic_canon, device, pk_out, vk_out, false);
} ZK_GUARD
extern "C" int zk_keygen_full(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t nIn, uint32_t V,
                              const uint64_t toxic_canon[20], int device, zk_pk **pk_out, zk_vk **vk_out) try {
    return keygen_impl(A, B, C, nC, nIn, V, toxic_canon, device, pk_out, vk_out, true);
} ZK_GUARD

// ================================================================ witness completion on the GPU
// The reference fills pb.values on the host, gadget by gadget (generate_r1cs_witness).  For circuits whose constraints are in
// "solved order" -- every constraint reads known variables in A and B and introduces at most ONE new variable, linearly, in C;
// true of the MiMC / Merkle gadgets and of the synthetic chain -- the constraint system itself is the witness program:
//     w[t_j] = (<A_j, w> <B_j, w> - sum_{i != t_j} C_ji w_i) / C_{j t_j}
// A plan (zk_wplan) is that program compiled once; zk_wplan_solve runs it for k witnesses at a time, one thread per witness
// (the k threads walk the same constraints in lock step: no divergence), directly in the buffer zk_prove_batch_submit_resident
// then proves from -- the witnesses never visit the host.  Constraints that introduce nothing are checked instead.
// Round 3: the program is a TAPE.  The first version walked the three CSR matrices (row pointers -> column / coefficient -> witness
// value: three dependent global-load round trips per constraint, 3 us each, 62-72 ms for the 21 345 constraints of the depth-29 Merkle
// circuit whatever k).  The tape is a sequence of fixed-size records of WP_WORDS 32-bit words that the wave reads with SCALAR loads (every
// lane = witness executes the same record; a record's address does not depend on data, so the next one is in flight while this one is
// evaluated):
//     word 0   nA | nB << 8 | nC << 16 | has_inverse << 24 | partial << 25     (terms held by THIS record: nA, nB <= 3, nC <= 2)
//     word 1   target variable (0xffffffff: nothing introduced, check)          word 2   index of 1 / C_{j,target} in the coefficient table
//     word 3   cache slot the result goes to
//     words 4..9 the A terms, 10..15 the B terms, 16..19 the C terms, two words each:
//     term.0   column | kind << 28 | fill << 30     kind 0: + w, 1: - w, 2: + coef w (a product), 3: + coef (a term on the constant ONE)
//     term.1   coefficient index | (slot + 1) << 24  slot + 1 = 0: load w[column] from memory (fill: and keep it in the slot given), else
//                                                    the value is in that slot of the cache
// A constraint with longer linear combinations spans several records (partial = 1 on all but the last: the sums carry over).
// The cache is WP_SLOTS witness values per lane in LDS, managed at COMPILE time (least recently used): the kernel indexes it with the
// slot number the tape names -- a dynamically indexed register file -- so a chain of constraints (MiMC: every constraint reads the one or
// two before it, every round the key) never waits for its own store to come back from memory; what remains per constraint is about one
// Montgomery product and one or two additions of a lone wave, ~410 VALU instructions (SQ counters).
namespace {
constexpr uint32_t WP_SLOTS = 32, WP_WORDS = 20, WP_A = 4, WP_B = 10, WP_C = 16, WP_NA = 3, WP_NB = 3, WP_NC = 2;
__global__ void __launch_bounds__(64)
k_witness_tape(const uint32_t *__restrict__ tape, uint32_t n_records, const fe *__restrict__ coefs,
               fe *__restrict__ w, uint32_t stride, uint32_t k, uint32_t *__restrict__ violations) {
    __shared__ uint32_t cache[WP_SLOTS][8][64];                  // [slot][limb][lane]: conflict-free, 64 KiB
    const uint32_t lane = threadIdx.x, p = blockIdx.x * blockDim.x + lane;
    const bool live = p < k;
    fe *x = w + (size_t)(live ? p : 0) * stride;                 // (idle lanes of the last wave shadow witness 0 and store nothing)
    fe lcA = Fr::zero(), lcB = lcA, lcC = lcA;
    bool eA = true, eB = true, eC = true;                        // (uniform) the sums are still empty: the first term is moved, not added
    uint32_t bad = 0;
    auto cache_get = [&](uint32_t slot) { fe v;
#pragma unroll
        for (int l = 0; l < 8; l++) v.l[l] = cache[slot][l][lane];
        return v; };
    auto cache_put = [&](uint32_t slot, const fe &v) {
#pragma unroll
        for (int l = 0; l < 8; l++) cache[slot][l][lane] = v.l[l]; };
    // general coefficients (kind 2: a product per term) and inverses are rare in gadget circuits (none in the MiMC / Merkle ones): one
    // shared, out-of-line product site keeps the straight-line code of the eight term slots small
    fe gen_v = lcA; uint32_t gen_c = 0;
    auto GENERAL = [&]() __attribute__((noinline)) { gen_v = Fr::mul(coefs[gen_c], gen_v); };
    // (requesting all operands of a record first and folding them afterwards -- two sweeps -- was measured: 39 ms against 35.6)
#define ZK_WP_TERM(ACC, EMPTY, W0, W1) { \
        const uint32_t t0_ = (W0), t1_ = (W1), kind_ = (t0_ >> 28) & 3u, slot1_ = (t1_ >> 24) & 0x3fu; \
        fe v_; \
        if (kind_ == 3) v_ = coefs[t1_ & 0xffffffu]; \
        else if (slot1_ && !((t0_ >> 30) & 1u)) v_ = cache_get(slot1_ - 1); \
        else { v_ = x[t0_ & 0x0fffffffu]; if (slot1_) cache_put(slot1_ - 1, v_); } \
        if (kind_ == 2) { gen_v = v_; gen_c = t1_ & 0xffffffu; GENERAL(); v_ = gen_v; } \
        if (EMPTY) { ACC = kind_ == 1 ? Fr::neg(v_) : v_; EMPTY = false; } \
        else ACC = kind_ == 1 ? Fr::sub(ACC, v_) : Fr::add(ACC, v_); }
    uint32_t nx[WP_WORDS];                                       // the NEXT record, requested one iteration ahead (scalar registers)
#pragma unroll
    for (uint32_t i = 0; i < WP_WORDS; i++) nx[i] = tape[i];
    for (uint32_t j = 0; j < n_records; j++) {
        uint32_t rec[WP_WORDS];
#pragma unroll
        for (uint32_t i = 0; i < WP_WORDS; i++) rec[i] = nx[i];
        const uint32_t *nrec = tape + (size_t)(j + 1) * WP_WORDS;     // (the tape ends in empty records: reading ahead is safe)
#pragma unroll
        for (uint32_t i = 0; i < WP_WORDS; i++) nx[i] = nrec[i];
        const uint32_t head = rec[0], target = rec[1], inv_idx = rec[2], out_slot = rec[3];
        if ((head >> 26) & 1u) {                                 // HINT record (zk_wplan_create_hinted): values the constraints only CHECK
            // ZK_WHINT_BITS: w[first + i] = bit i of the canonical value of w[src], i < count (field2bits-style gadgets: the bits are
            // non-deterministic advice, the constraints b (1 - b) = 0 and sum 2^i b_i = x that follow verify them)
            // ZK_WHINT_INV / ZK_WHINT_NONZERO (bits 27-28 = 1 / 2): w[first] = 1 / w[src] (0 for 0: 0^(r-2) = 0), resp. [w[src] != 0] -- the M and Y of
            // the reference's IsNonZero gadget (src/gadgets/isnonzero.cpp:48-60), whose three constraints only check them
            const uint32_t src = target, first = inv_idx, count = out_slot, hk = (head >> 27) & 3u;
            const fe one = Fr::one(), zero = Fr::zero();
            if (hk == 0) {
                const fe v = Fr::from_mont(x[src]);
                if (live) for (uint32_t i = 0; i < count; i++) x[first + i] = (i < 256 && ((v.l[i >> 5] >> (i & 31)) & 1u)) ? one : zero;
            } else {
                const fe v = x[src];
                const fe r = hk == 1 ? Fr::inv(v) : (Fr::is_zero(v) ? zero : one);
                if (live) x[first] = r;
            }
            continue;
        }
        const uint32_t nA = head & 0xffu, nB = (head >> 8) & 0xffu, nC = (head >> 16) & 0xffu;
        if (nA > 0) ZK_WP_TERM(lcA, eA, rec[WP_A + 0], rec[WP_A + 1])
        if (nA > 1) ZK_WP_TERM(lcA, eA, rec[WP_A + 2], rec[WP_A + 3])
        if (nA > 2) ZK_WP_TERM(lcA, eA, rec[WP_A + 4], rec[WP_A + 5])
        if (nB > 0) ZK_WP_TERM(lcB, eB, rec[WP_B + 0], rec[WP_B + 1])
        if (nB > 1) ZK_WP_TERM(lcB, eB, rec[WP_B + 2], rec[WP_B + 3])
        if (nB > 2) ZK_WP_TERM(lcB, eB, rec[WP_B + 4], rec[WP_B + 5])
        if (nC > 0) ZK_WP_TERM(lcC, eC, rec[WP_C + 0], rec[WP_C + 1])
        if (nC > 1) ZK_WP_TERM(lcC, eC, rec[WP_C + 2], rec[WP_C + 3])
        if ((head >> 25) & 1u) continue;                         // partial record: the constraint's sums go on in the next one
        fe v = (eA || eB) ? Fr::zero() : Fr::mul(lcA, lcB);      // an empty sum is 0
        if (!eC) v = Fr::sub(v, lcC);
        eA = eB = eC = true;
        if (target == 0xffffffffu) { bad += live && !Fr::is_zero(v); continue; }
        if ((head >> 24) & 1u) { gen_v = v; gen_c = inv_idx; GENERAL(); v = gen_v; }
        if (live) x[target] = v;
        cache_put(out_slot, v);
    }
#undef ZK_WP_TERM
    if (bad) atomicAdd(violations, bad);
}
}  // namespace

struct zk_wplan {
    int device = 0;
    uint32_t nC = 0, V = 0, n_records = 0;                           // (a wide plan: its program is the tape, its passes the records)
    size_t n_words = 0, n_coefs = 0;                                 // what d_tape and d_coefs hold (zk_wplan_probe_program)
    zk_wplan_stats stats = {};                                       // kind 0: tape, 1: wide (wplan_wide.hpp)
    uint32_t *d_tape = nullptr, *d_viol = nullptr;
    fe *d_coefs = nullptr;
    hipStream_t st = nullptr;
    ~zk_wplan() {
        DeviceScope on(device);
        if (d_tape) hipFree(d_tape);
        if (d_viol) hipFree(d_viol);
        if (d_coefs) hipFree(d_coefs);
        if (st) hipStreamDestroy(st);
    }
};

#include "wplan_wide.hpp"

extern "C" int zk_wplan_create(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V,
                               const uint8_t *known, int device, zk_wplan **out) try {
    return zk_wplan_create_hinted(A, B, C, nC, V, known, nullptr, 0, device, out);
} ZK_GUARD
extern "C" int zk_wplan_create_hinted(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V,
                                      const uint8_t *known, const zk_whint *hints, uint32_t n_hints, int device, zk_wplan **out) try {
    if (!A || !B || !C || !known || !out || (n_hints && !hints)) return fail(ZK_ERR_ARG, "null argument");
    if (A->n_rows != nC || B->n_rows != nC || C->n_rows != nC) return fail(ZK_ERR_ARG, "CSR row counts must equal nC");
    if (V >= (1u << 28)) return fail(ZK_ERR_ARG, "witness plan: more than 2^28 variables");
    ZK_TRY(use_device(device));
    std::vector<uint8_t> have(known, known + (size_t)V + 1);
    have[0] = 1;                                                     // the constant ONE
    std::vector<uint32_t> tape;
    uint32_t products = 0;                                           // (zk_wplan_info: field products per witness)
    std::vector<fe> coefs;                                           // distinct coefficients (and inverses), Montgomery
    auto coef_index = [&](const fe &c) -> uint32_t {                 // (linear search from the back: gadget circuits reuse few values)
        for (size_t i = coefs.size(); i-- > 0 && coefs.size() - i <= 64;) if (Fr::eq(coefs[i], c)) return (uint32_t)i;
        coefs.push_back(c); return (uint32_t)coefs.size() - 1;
    };
    const fe one = Fr::one(), minus_one = Fr::neg(one);
    // hints: variable -> the hint that defines it; a hint runs right before the first constraint that reads one of its variables
    std::vector<uint32_t> hint_of((size_t)V + 1, 0xffffffffu);
    std::vector<uint8_t> hint_done(n_hints, 0);
    for (uint32_t h = 0; h < n_hints; h++) {
        if (hints[h].kind != ZK_WHINT_BITS && hints[h].kind != ZK_WHINT_INV && hints[h].kind != ZK_WHINT_NONZERO) return fail(ZK_ERR_ARG, "witness plan: unknown hint kind");
        if (hints[h].kind != ZK_WHINT_BITS && hints[h].count != 1) return fail(ZK_ERR_ARG, "witness plan: ZK_WHINT_INV / ZK_WHINT_NONZERO define one variable (count = 1)");
        if (hints[h].src > V || hints[h].count == 0 || (uint64_t)hints[h].first + hints[h].count > (uint64_t)V + 1 || hints[h].first == 0) return fail(ZK_ERR_ARG, "witness plan: hint variables out of range");
        for (uint32_t i = 0; i < hints[h].count; i++) {
            if (have[hints[h].first + i] || hint_of[hints[h].first + i] != 0xffffffffu) return fail(ZK_ERR_ARG, "witness plan: a hint defines a variable that is supplied or defined twice");
            hint_of[hints[h].first + i] = h;
        }
    }
    char msg[200];
    auto try_hint = [&](uint32_t v) -> bool {                      // can a hint supply v now?  then emit its record
        const uint32_t h = v <= V ? hint_of[v] : 0xffffffffu;
        if (h == 0xffffffffu || hint_done[h] || !have[hints[h].src]) return false;
        uint32_t rec[WP_WORDS] = {0};
        rec[0] = 1u << 26 | (hints[h].kind - ZK_WHINT_BITS) << 27; rec[1] = hints[h].src; rec[2] = hints[h].first; rec[3] = hints[h].count;
        tape.insert(tape.end(), rec, rec + WP_WORDS);
        for (uint32_t i = 0; i < hints[h].count; i++) have[hints[h].first + i] = 1;      // (in memory only: the first read of each goes through the cache fill)
        hint_done[h] = 1;
        return true;
    };
    // the kernel's per-lane cache of WP_SLOTS witness values, simulated here: which variable sits in which slot, least recently used out
    uint32_t slot_var[WP_SLOTS]; uint64_t slot_used[WP_SLOTS]; uint64_t tick = 0;
    for (uint32_t i = 0; i < WP_SLOTS; i++) { slot_var[i] = 0xffffffffu; slot_used[i] = 0; }
    auto cache_find = [&](uint32_t v) -> int { for (uint32_t i = 0; i < WP_SLOTS; i++) if (slot_var[i] == v) { slot_used[i] = ++tick; return (int)i; } return -1; };
    auto cache_alloc = [&](uint32_t v) -> uint32_t { uint32_t best = 0; for (uint32_t i = 1; i < WP_SLOTS; i++) if (slot_used[i] < slot_used[best]) best = i;
                                                     slot_var[best] = v; slot_used[best] = ++tick; return best; };
    for (uint32_t j = 0; j < nC; j++) {
        const zk_csr *M[2] = {A, B};
        for (int q = 0; q < 2; q++)
            for (uint32_t e = M[q]->row_ptr[j]; e < M[q]->row_ptr[j + 1]; e++) {
                if (M[q]->col[e] > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables");
                if (!have[M[q]->col[e]]) try_hint(M[q]->col[e]);
                if (!have[M[q]->col[e]]) { snprintf(msg, sizeof(msg), "constraint %u reads variable %u in %c before anything defines it: not in solved order", j, M[q]->col[e], q ? 'B' : 'A'); return fail(ZK_ERR_ARG, msg); }
            }
        uint32_t target = 0xffffffffu; fe tcoef = one;
        for (uint32_t e = C->row_ptr[j]; e < C->row_ptr[j + 1]; e++) {
            const uint32_t v = C->col[e];
            if (v > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables");
            if (!have[v]) try_hint(v);
            if (have[v]) continue;
            if (target != 0xffffffffu) { snprintf(msg, sizeof(msg), "constraint %u introduces two new variables (%u and %u)", j, target, v); return fail(ZK_ERR_ARG, msg); }
            fe cf; memcpy(cf.l, C->coeff + 4 * (size_t)e, 32);
            if (Fr::is_zero(cf)) return fail(ZK_ERR_ARG, "zero coefficient on the variable a constraint introduces");
            target = v; tcoef = cf;
        }
        const bool has_inv = target != 0xffffffffu && !Fr::eq(tcoef, one);
        const uint32_t inv_idx = has_inv ? coef_index(Fr::inv(tcoef)) : 0u;
        // the constraint's terms, encoded, per linear combination
        std::vector<uint32_t> terms[3];
        const zk_csr *Ms[3] = {A, B, C};
        for (int q = 0; q < 3; q++)
            for (uint32_t e = Ms[q]->row_ptr[j]; e < Ms[q]->row_ptr[j + 1]; e++) {
                const uint32_t col = Ms[q]->col[e];
                if (q == 2 && col == target) continue;
                fe cf; memcpy(cf.l, Ms[q]->coeff + 4 * (size_t)e, 32);
                if (Fr::is_zero(cf)) continue;
                uint32_t kind, ci = 0;
                if (col == 0) { kind = 3; ci = coef_index(cf); }                    // coef * ONE: the coefficient itself
                else if (Fr::eq(cf, one)) kind = 0;
                else if (Fr::eq(cf, minus_one)) kind = 1;
                else { kind = 2; ci = coef_index(cf); products++; }
                if (ci >= (1u << 24)) return fail(ZK_ERR_ARG, "witness plan: more than 2^24 distinct coefficients");
                terms[q].push_back(col | kind << 28);                               // (the cache slot is decided when the term's record is laid out)
                terms[q].push_back(ci);
            }
        products += (!terms[0].empty() && !terms[1].empty()) + has_inv;
        // records of at most WP_NA / WP_NB / WP_NC terms; all but the last are partial
        size_t done[3] = {0, 0, 0};
        for (;;) {
            uint32_t rec[WP_WORDS] = {0};
            const uint32_t cap[3] = {WP_NA, WP_NB, WP_NC}, at[3] = {WP_A, WP_B, WP_C};
            uint32_t n[3];
            bool more = false;
            for (int q = 0; q < 3; q++) {
                const size_t left = terms[q].size() / 2 - done[q];
                n[q] = (uint32_t)(left < cap[q] ? left : cap[q]);
                for (uint32_t t = 0; t < n[q]; t++) {               // the cache is simulated in the order the kernel evaluates: record by record
                    uint32_t w0 = terms[q][2 * (done[q] + t)], w1 = terms[q][2 * (done[q] + t) + 1];
                    if (((w0 >> 28) & 3u) != 3) {
                        const uint32_t col = w0 & 0x0fffffffu;
                        const int hit = cache_find(col);
                        if (hit >= 0) w1 |= ((uint32_t)hit + 1) << 24;
                        else { w1 |= (cache_alloc(col) + 1) << 24; w0 |= 1u << 30; }    // from memory this once (fill), then from the cache
                    }
                    rec[at[q] + 2 * t] = w0; rec[at[q] + 2 * t + 1] = w1;
                }
                done[q] += n[q];
                more |= done[q] < terms[q].size() / 2;
            }
            rec[0] = n[0] | n[1] << 8 | n[2] << 16 | (has_inv ? 1u << 24 : 0u) | (more ? 1u << 25 : 0u);
            rec[1] = target; rec[2] = inv_idx;
            if (!more && target != 0xffffffffu) rec[3] = cache_alloc(target);       // where the result is kept
            tape.insert(tape.end(), rec, rec + WP_WORDS);
            if (!more) break;
        }
        if (target != 0xffffffffu) have[target] = 1;
    }
    for (uint32_t v = 0; v <= V; v++) if (!have[v]) { snprintf(msg, sizeof(msg), "variable %u is neither supplied nor defined by a constraint", v); return fail(ZK_ERR_ARG, msg); }
    const uint32_t n_records = (uint32_t)(tape.size() / WP_WORDS);
    tape.insert(tape.end(), 3 * WP_WORDS, 0u);                       // the read-ahead past the last record finds empty records
    if (coefs.empty()) coefs.push_back(one);
    std::unique_ptr<zk_wplan> p(new zk_wplan());
    p->device = device; p->nC = nC; p->V = V; p->n_records = n_records;
    p->stats.records_or_passes = n_records; p->stats.products = products;
    int rc = dev_upload(&p->d_tape, tape.data(), tape.size());
    if (rc == ZK_OK) rc = dev_upload(&p->d_coefs, coefs.data(), coefs.size());
    if (rc == ZK_OK && hipMalloc(&p->d_viol, 4) != hipSuccess) rc = ZK_ERR_NOMEM;
    if (rc == ZK_OK && hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking) != hipSuccess) rc = ZK_ERR_HIP;
    if (rc != ZK_OK) return rc;
    *out = p.release();
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_wplan_create_wide(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V, const uint8_t *known,
                                    const zk_whint *hints, uint32_t n_hints, uint32_t lanes, int device, zk_wplan **out) try {
    if (!A || !B || !C || !known || !out || (n_hints && !hints)) return fail(ZK_ERR_ARG, "null argument");
    if (A->n_rows != nC || B->n_rows != nC || C->n_rows != nC) return fail(ZK_ERR_ARG, "CSR row counts must equal nC");
    if (V >= (1u << 28)) return fail(ZK_ERR_ARG, "witness plan: more than 2^28 variables");
    if (lanes < 4 || lanes > 64 || (lanes & (lanes - 1))) return fail(ZK_ERR_ARG, "witness plan (wide): lanes must be 4, 8, 16, 32 or 64");
    ZK_TRY(use_device(device));
    WidePlanHost h;
    ZK_TRY(wide_compile(A, B, C, nC, V, known, hints, n_hints, lanes, h));
    std::unique_ptr<zk_wplan> p(new zk_wplan());
    p->device = device; p->nC = nC; p->V = V; p->n_records = h.st.records_or_passes; p->stats = h.st;
    p->n_words = h.prog.size(); p->n_coefs = h.coefs.size();
    int rc = dev_upload(&p->d_tape, h.prog.data(), h.prog.size());
    if (rc == ZK_OK) rc = dev_upload(&p->d_coefs, h.coefs.data(), h.coefs.size());
    if (rc == ZK_OK && hipMalloc(&p->d_viol, 4) != hipSuccess) rc = ZK_ERR_NOMEM;
    if (rc == ZK_OK && hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking) != hipSuccess) rc = ZK_ERR_HIP;
    if (rc != ZK_OK) return rc;
    *out = p.release();
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_wplan_info(const zk_wplan *p, zk_wplan_stats *out) try {
    if (!p || !out) return fail(ZK_ERR_ARG, "null argument");
    *out = p->stats;
    return ZK_OK;
} ZK_GUARD
extern "C" void zk_wplan_free(zk_wplan *p) try { delete p; } ZK_GUARD_VOID
// TEST INFRASTRUCTURE: what a wide plan uploaded, read back from device memory -- the pass records ([pass][word][lane in group], the empty
// last pass included), then the coefficient table the records index (8 words per entry, Montgomery).  *n_words is set whenever the plan is
// a wide one, so a caller can size its buffer from a first call with cap = 0.
extern "C" int zk_wplan_probe_program(const zk_wplan *p, uint32_t *words, size_t cap, size_t *n_words) try {
    if (!p || !n_words) return fail(ZK_ERR_ARG, "null argument");
    if (p->stats.kind != 1) return fail(ZK_ERR_ARG, "witness plan probe: a tape plan has no lane program");
    const size_t n = p->n_words + 8 * p->n_coefs;
    *n_words = n;
    if (!words || cap < n) return fail(ZK_ERR_ARG, "witness plan probe: the buffer is shorter than the program");
    ZK_TRY(use_device(p->device));
    ZK_HIP(hipMemcpy(words, p->d_tape, 4 * p->n_words, hipMemcpyDeviceToHost));
    ZK_HIP(hipMemcpy(words + p->n_words, p->d_coefs, 32 * p->n_coefs, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD
// d_w: k witnesses, (V + 1) x 32 bytes each, contiguous, device memory, Montgomery; the supplied variables (and ONE at index
// 0) filled in.  Completes them in place; *violations = constraints (over all k) that introduce nothing and do not hold.
extern "C" int zk_wplan_solve(zk_wplan *p, void *d_w, uint32_t k, uint32_t *violations) try {
    if (!p || !d_w || !k) return fail(ZK_ERR_ARG, "bad argument");
    ZK_TRY(use_device(p->device));
    ZK_HIP(hipMemsetAsync(p->d_viol, 0, 4, p->st));
    if (p->stats.kind == 1) {                                        // wide plan: a wave holds 64 / lanes witnesses
        const uint32_t lanes_log2 = (uint32_t)__builtin_ctz(p->stats.lanes);
        ZK_LAUNCH_SYNC(k_witness_wide, zk_div_up(k, 64u >> lanes_log2), 64, p->st, (const uint32_t *)p->d_tape, p->n_records, (const fe *)p->d_coefs, (fe *)d_w, p->V + 1, k, lanes_log2, p->d_viol);
    } else
    ZK_LAUNCH(k_witness_tape, zk_div_up(k, 64), 64, p->st, (const uint32_t *)p->d_tape, p->n_records, (const fe *)p->d_coefs, (fe *)d_w, p->V + 1, k, p->d_viol);
    uint32_t v = 0;
    ZK_HIP(hipMemcpyAsync(&v, p->d_viol, 4, hipMemcpyDeviceToHost, p->st));
    ZK_HIP(hipStreamSynchronize(p->st));
    if (violations) *violations = v;
    return ZK_OK;
} ZK_GUARD
// plain device-memory helpers for hosts that have no HIP binding of their own (tests, ctypes clients)
extern "C" int zk_dev_alloc(size_t bytes, int device, void **out) try {
    if (!out) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(device));
    ZK_HIP(hipMalloc(out, bytes ? bytes : 1));
    return ZK_OK;
} ZK_GUARD
extern "C" int zk_dev_free(void *p) try { return (!p || hipFree(p) == hipSuccess) ? ZK_OK : ZK_ERR_HIP; } ZK_GUARD
extern "C" int zk_dev_upload(void *dst, const void *src, size_t bytes) try { if (!dst || !src) return fail(ZK_ERR_ARG, "null argument"); ZK_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return ZK_OK; } ZK_GUARD
extern "C" int zk_dev_download(void *dst, const void *src, size_t bytes) try { if (!dst || !src) return fail(ZK_ERR_ARG, "null argument"); ZK_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return ZK_OK; } ZK_GUARD

// ================================================================ JSON (src/export.cpp:20-121)
namespace {
// HexStringFromBigint = mpz_get_str(., 16, .): lowercase, no leading zeros, zero prints "0"
void hex_canon(std::string &s, const uint64_t v[4]) {
    bool started = false;
    for (int i = 3; i >= 0; i--) for (int sh = 60; sh >= 0; sh -= 4) {
        unsigned d = (unsigned)(v[i] >> sh) & 15u;
        if (d || started) { s.push_back("0123456789abcdef"[d]); started = true; }
    }
    if (!started) s.push_back('0');
}
void q(std::string &s, const uint64_t v[4]) { s += "\"0x"; hex_canon(s, v); s += "\""; }
}  // namespace

extern "C" int zk_proof_to_json(const zk_proof *p, const uint64_t *inputs, uint32_t nIn, int canonical,
                                char *buf, size_t cap, size_t *len) try {
    if (!p || (nIn && !inputs) || !len) return fail(ZK_ERR_ARG, "null argument");
    std::string s;
    s.reserve(1024 + 70 * (size_t)nIn);
    s += "{\n \"A\" :["; q(s, p->a_x); s += ", "; q(s, p->a_y);
    s += "],\n \"B\"  :[["; q(s, p->b_x_c1); s += ", "; q(s, p->b_x_c0); s += "],\n ["; q(s, p->b_y_c1); s += ", "; q(s, p->b_y_c0);
    s += "]],\n \"C\"  :["; q(s, p->c_x); s += ", "; q(s, p->c_y);
    s += "],\n \"input\" :[";
    for (uint32_t i = 0; i < nIn; i++) {
        uint64_t v[4];
        fe e; memcpy(e.l, inputs + 4 * (size_t)i, 32);
        if (!canonical) e = Fr::from_mont(e);
        memcpy(v, e.l, 32);
        q(s, v);
        if (i + 1 < nIn) s += ", ";
    }
    s += "]\n}";
    *len = s.size();
    if (!buf || cap < s.size() + 1) return fail(ZK_ERR_BUFFER, "JSON buffer too small");
    memcpy(buf, s.data(), s.size()); buf[s.size()] = 0;
    return ZK_OK;
} ZK_GUARD


// vk2json, src/export.cpp:124-145
extern "C" int zk_vk_to_json(const zk_vk *vk, char *buf, size_t cap, size_t *len) try {
    if (!vk || !len) return fail(ZK_ERR_ARG, "null argument");
    std::string s;
    auto g1 = [&](const G1::Affine &p) {
        uint64_t x[4], y[4]; uint32_t inf;
        put_g1(G1::from_affine(p), x, y, &inf);
        q(s, x); s += ", "; q(s, y);
    };
    auto g2 = [&](const G2::Affine &p) {
        uint64_t a[4], b[4], c[4], d[4]; uint32_t inf;
        put_g2(G2::from_affine(p), a, b, c, d, &inf);
        s += "["; q(s, b); s += ", "; q(s, a); s += "],\n ["; q(s, d); s += ", "; q(s, c); s += "]";
    };
    s += "{\n \"alpha\" :["; g1(vk->alpha_g1);
    s += "],\n \"beta\"  :["; g2(vk->beta_g2);
    s += "],\n \"gamma\" :["; g2(vk->gamma_g2);
    s += "],\n \"delta\" :["; g2(vk->delta_g2);
    s += "],\n\"gammaABC\" :[[";
    for (size_t i = 0; i < vk->gamma_abc.size(); i++) { if (i) s += ",["; g1(vk->gamma_abc[i]); s += "]"; }
    s += "]}";
    *len = s.size();
    if (!buf || cap < s.size() + 1) return fail(ZK_ERR_BUFFER, "JSON buffer too small");
    memcpy(buf, s.data(), s.size()); buf[s.size()] = 0;
    return ZK_OK;
} ZK_GUARD

// ================================================================ kernel-level entry points (tests / micro-benchmarks)
extern "C" int zk_ntt(uint64_t *data, uint32_t logm, int inverse, int coset, int device) try {
    if (!data || logm > 28) return fail(ZK_ERR_ARG, "bad argument");
    ZK_TRY(use_device(device));
    NttTables tab; fe *d_in = nullptr, *d_out = nullptr;
    const size_t bytes = 32ull << logm;
    int rc = ntt_tables_create(tab, logm, nullptr);
    if (rc == ZK_OK && hipMalloc(&d_in, bytes) != hipSuccess) rc = ZK_ERR_NOMEM;
    if (rc == ZK_OK && hipMalloc(&d_out, bytes) != hipSuccess) rc = ZK_ERR_NOMEM;
    if (rc == ZK_OK && hipMemcpy(d_in, data, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = ZK_ERR_HIP;
    if (rc == ZK_OK) {
        const fe *pre = (!inverse && coset) ? tab.coset_fwd : nullptr;
        const fe *post = inverse ? (coset ? tab.icoset : tab.inv_m) : nullptr;
        rc = ntt_run(tab, d_in, d_out, inverse != 0, pre, post, nullptr);
    }
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "NTT kernels failed");
    if (rc == ZK_OK && hipMemcpy(data, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_ERR_HIP;
    if (d_in) hipFree(d_in);
    if (d_out) hipFree(d_out);
    ntt_tables_free(tab);
    return rc;
} ZK_GUARD

// TEST INFRASTRUCTURE: ONE ntt_run over the production tables with the batch, stride and fused steps of the caller's choice (include/zkhip.h)
extern "C" int zk_ntt_probe(const uint64_t *in, const uint64_t *in2, const uint64_t *sub, uint64_t *out, uint32_t logm, uint32_t batch, uint32_t stride,
                            int inverse, int pre, int post, int post_alt, uint32_t alt_from, int device) try {
    if (!in || !out) return fail(ZK_ERR_ARG, "transform probe: null argument");
    if (logm > 28) return fail(ZK_ERR_ARG, "transform probe: logm above 28");
    if (!batch) return fail(ZK_ERR_ARG, "transform probe: batch = 0");
    if (stride < (1u << logm)) return fail(ZK_ERR_ARG, "transform probe: stride below m");
    if (pre < 0 || pre > 1 || post < 0 || post > 5 || post_alt < 0 || post_alt > 5) return fail(ZK_ERR_ARG, "transform probe: unknown scaling table");
    if (sub && !post) return fail(ZK_ERR_ARG, "transform probe: sub needs post (k_ntt_pass)");
    ZK_TRY(use_device(device));
    NttTables tab; fe *d_in = nullptr, *d_out = nullptr, *d_in2 = nullptr, *d_sub = nullptr;
    const size_t n = (size_t)batch * stride;                    // every array is copied whole, gaps between the vectors included
    int rc = ntt_tables_create(tab, logm, nullptr);
    if (rc == ZK_OK) rc = dev_upload(&d_in, (const fe *)in, n);
    if (rc == ZK_OK) rc = dev_upload(&d_out, (const fe *)out, n);   // the caller's output comes back as it was wherever the transform does not write
    if (rc == ZK_OK && in2) rc = dev_upload(&d_in2, (const fe *)in2, n);
    if (rc == ZK_OK && sub) rc = dev_upload(&d_sub, (const fe *)sub, n);
    if (rc == ZK_OK) {
        const fe *scale[6] = {nullptr, tab.inv_m, tab.icoset, tab.inv_then_coset, tab.inv_m_zinv, tab.icoset_zinv};
        NttFuse fuse; fuse.in2 = d_in2; fuse.sub = d_sub; fuse.post_alt = scale[post_alt]; fuse.alt_from = alt_from;
        rc = ntt_run(tab, d_in, d_out, inverse != 0, pre ? tab.coset_fwd : nullptr, scale[post], nullptr, batch, stride, fuse);
    }
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "NTT kernels failed");
    if (rc == ZK_OK && hipMemcpy(out, d_out, 32 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_ERR_HIP;
    fe *bufs[] = {d_in, d_out, d_in2, d_sub};
    for (fe *p : bufs) if (p) hipFree(p);
    ntt_tables_free(tab);
    return rc;
} ZK_GUARD

extern "C" int zk_witness_map(zk_ctx *c, const uint64_t *witness, int canonical, uint64_t *h_out) try {
    if (!c || !witness || !h_out) return fail(ZK_ERR_ARG, "null argument");
    if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is in flight on this context (collect it first): its witness and H buffers are in use");
    ZK_TRY(use_device(c->device));
    c->cur_batch = 1;
    ZK_TRY(upload_witness(c, witness, canonical));
    ZK_TRY(enqueue_compute_h(c, c->s_main));
    ZK_HIP(hipStreamSynchronize(c->s_main));
    ZK_HIP(hipMemcpy(h_out, c->d_t, 32 * (size_t)c->m, hipMemcpyDeviceToHost));
    memset(h_out + 4 * (size_t)c->m, 0, 32);
    return ZK_OK;
} ZK_GUARD

// TEST INFRASTRUCTURE: the row evaluations of a batch as the kernels left them (include/zkhip.h)
extern "C" int zk_ctx_probe_rows(zk_ctx *c, const uint64_t *witnesses, uint32_t k, int canonical, uint64_t *out) try {
    if (!c || !witnesses || !out) return fail(ZK_ERR_ARG, "null argument");
    if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is in flight on this context (collect it first): its witness and row buffers are in use");
    if (!k || k > c->max_batch) return fail(ZK_ERR_ARG, "batch size exceeds zk_config.max_batch of this context");
    ZK_TRY(use_device(c->device));
    c->cur_batch = k;
    ZK_TRY(upload_witness(c, witnesses, canonical));
    ZK_TRY(enqueue_rows(c, c->s_main));
    ZK_HIP(hipStreamSynchronize(c->s_main));
    ZK_HIP(hipMemcpy(out, c->d_a, 3 * 32 * (size_t)c->m * k, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_GUARD

// TEST INFRASTRUCTURE: the context's own H pipeline on a batch, and what each of its steps left (include/zkhip.h)
extern "C" int zk_ctx_probe_h(zk_ctx *c, const uint64_t *witnesses, uint32_t k, int canonical, uint64_t *first, uint64_t *coset, uint64_t *last,
                              uint64_t *hpart, uint64_t *tail, uint64_t *h_tail, uint32_t info[8]) try {
    if (!c || !witnesses || !first || !coset || !last || !hpart || !tail || !h_tail || !info) return fail(ZK_ERR_ARG, "null argument");
    if (c->in_flight) return fail(ZK_ERR_ARG, "a proof is in flight on this context (collect it first): its witness and H buffers are in use");
    if (!k || k > c->max_batch) return fail(ZK_ERR_ARG, "batch size exceeds zk_config.max_batch of this context");
    ZK_TRY(use_device(c->device));
    const uint32_t m = c->m, grid = c->lag ? zk_div_up(m, HL_PROD_THREADS * HL_PROD_PER) : 0;
    const size_t mk = (size_t)m * k;
    // the copies land in buffers of the probe's own and reach the caller's only after everything succeeded
    std::vector<fe> b_first((c->lag ? 2 : 3) * mk), b_coset(2 * mk), b_last(mk), b_hpart(2 * (size_t)grid * k), b_tail(c->lag ? k : 0);
    HSnap snap{b_first.data(), b_coset.data(), b_last.data(), c->lag ? b_hpart.data() : nullptr, c->lag ? b_tail.data() : nullptr};
    c->cur_batch = k;
    int rc = upload_witness(c, witnesses, canonical);
    if (rc == ZK_OK) rc = c->lag ? enqueue_compute_h4(c, c->s_main, &snap) : enqueue_compute_h(c, c->s_main, &snap);
    const hipError_t synced = hipStreamSynchronize(c->s_main);      // on every path: copies into the buffers above may be pending
    if (rc != ZK_OK) return rc;
    ZK_HIP(synced);
    memcpy(first, b_first.data(), 32 * b_first.size());
    memcpy(coset, b_coset.data(), 32 * b_coset.size());
    memcpy(last, b_last.data(), 32 * b_last.size());
    if (c->lag) { memcpy(hpart, b_hpart.data(), 32 * b_hpart.size()); memcpy(tail, b_tail.data(), 32 * b_tail.size()); }
    memcpy(h_tail, c->h_tail, 32 * (size_t)k);
    const uint32_t inf[8] = {c->lag ? 1u : 0u, m, k, grid, 0, 0, 0, 0};
    memcpy(info, inf, sizeof(inf));
    return ZK_OK;
} ZK_GUARD

template <class C>
static int msm_host(const uint64_t *bases, const uint64_t *scalars, uint32_t n, uint32_t cbits, int device, uint64_t *out_affine) {
    if ((n && (!bases || !scalars)) || !out_affine) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(device));
    typename C::Affine *d_bases = nullptr; fe *d_scalars = nullptr;
    MsmWork<C> work;
    int rc = dev_upload(&d_bases, (const typename C::Affine *)bases, n);
    if (rc == ZK_OK) rc = dev_upload(&d_scalars, (const fe *)scalars, n);
    uint32_t plog = 0;                                      // test aid: the frugal table layout (every 2^plog-th window, 2^plog bucket planes) at kernel level
    if (const char *e = getenv("ZK_TEST_PLANES_LOG")) plog = (uint32_t)atoi(e) & 7u;
    if (rc == ZK_OK) rc = work.alloc(n, cbits, nullptr, nullptr, false, 1, plog);
    if (rc == ZK_OK) rc = work.precompute(d_bases, n, nullptr);
    if (rc == ZK_OK) rc = work.enqueue(d_scalars, nullptr, n, 0, nullptr, nullptr);
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "MSM kernels failed");
    if (rc == ZK_OK) {
        typename C::Affine a = C::to_affine(work.finish());
        memcpy(out_affine, &a, sizeof(a));
    }
    work.release();
    if (d_bases) hipFree(d_bases);
    if (d_scalars) hipFree(d_scalars);
    return rc;
}
extern "C" int zk_msm_g1(const uint64_t *bases, const uint64_t *scalars, uint32_t n, uint32_t c, int device, uint64_t out[8]) try {
    return msm_host<G1>(bases, scalars, n, c, device, out);
} ZK_GUARD
extern "C" int zk_msm_g2(const uint64_t *bases, const uint64_t *scalars, uint32_t n, uint32_t c, int device, uint64_t out[16]) try {
    return msm_host<G2>(bases, scalars, n, c, device, out);
} ZK_GUARD

// TEST INFRASTRUCTURE: the bucket sort alone, off[] and sorted[] as k_sort_fine left them (include/zkhip.h).  A sort-only MsmWork as the
// shared witness sort of a context is one (zk_ctx_create: mW): no table, no curve arithmetic.
extern "C" int zk_msm_sort_probe(const uint64_t *scalars, uint32_t n, uint32_t batch, uint32_t stride, int canonical, uint32_t c, uint32_t plog,
                                 int shift_payload, int device, uint32_t *off, uint64_t off_cap, uint32_t *sorted, uint64_t sorted_cap, uint32_t info[16]) try {
    if (!off || !sorted || !info || (n && !scalars)) return fail(ZK_ERR_ARG, "null argument");
    if (!batch) return fail(ZK_ERR_ARG, "sort probe: batch = 0");
    if (stride < n) return fail(ZK_ERR_ARG, "sort probe: stride below n");
    if (plog > 7) return fail(ZK_ERR_ARG, "sort probe: plog above 7");
    if ((uint64_t)batch * stride >= (1ull << 32)) return fail(ZK_ERR_ARG, "sort probe: batch * stride must stay below 2^32");
    ZK_TRY(use_device(device));
    fe *d_scalars = nullptr;
    MsmWork<G1> work;
    uint64_t entries = 0;
    int rc = work.alloc(n, c, nullptr, nullptr, /*sort_only=*/true, batch, plog);
    const uint64_t nb = ((uint64_t)work.sh.nb * batch) << plog;          // buckets of the whole batch, all planes (enqueue_sort's nb)
    if (rc == ZK_OK && off_cap < nb + 1) rc = fail(ZK_ERR_ARG, "sort probe: off_cap below nb_total + 1");
    if (rc == ZK_OK) rc = dev_upload(&d_scalars, (const fe *)scalars, n ? (size_t)(batch - 1) * stride + n : 0);
    if (rc == ZK_OK && shift_payload) work.use_shift_payload();
    if (rc == ZK_OK) rc = work.enqueue_sort(d_scalars, nullptr, n, canonical, nullptr, batch, stride);
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "sort kernels failed");
    if (rc == ZK_OK && hipMemcpy(off, work.off, sizeof(uint32_t) * (nb + 1), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ZK_ERR_HIP, "sort probe: copying off[] back failed");
    if (rc == ZK_OK) {
        SortShape sq = work.ss; sq.resize(n * batch ? n * batch : 1, (uint32_t)nb);      // the shape enqueue_sort launched with
        entries = off[nb];
        const uint32_t v[16] = {work.sh.c, work.sh.W, (uint32_t)nb, sq.cb, sq.fb, sq.fine_bits, sq.groups, sq.per_group, work.sort_kbits,
                                work.sort_staged ? 1u : 0u, (uint32_t)entries, 0, 0, 0, 0, 0};
        memcpy(info, v, sizeof(v));
        if (entries > work.sh.max_entries() * batch) rc = fail(ZK_ERR_INTERNAL, "sort probe: off[nb_total] exceeds n * W * batch");   // nothing past the allocation is read back
        else if (entries > sorted_cap) rc = fail(ZK_ERR_ARG, "sort probe: sorted_cap below off[nb_total] (info[10])");
    }
    if (rc == ZK_OK && entries && hipMemcpy(sorted, work.sorted, sizeof(uint32_t) * entries, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ZK_ERR_HIP, "sort probe: copying sorted[] back failed");
    work.release();
    if (d_scalars) hipFree(d_scalars);
    return rc;
} ZK_GUARD

// TEST INFRASTRUCTURE: one multi-exponentiation stage by stage (include/zkhip.h).  The work objects are driven exactly as a context drives
// its own -- alloc, precompute, enqueue_sort, enqueue_accumulate, enqueue_tail -- and every buffer read back outlives those calls, so no
// kernel and no launch code knows about the probe.  Every copy is bounded by what the caller's capacity check (before any launch) and the
// allocation allow, never by a count that only the device supplied.
namespace {
template <class C> struct StageSide {
    MsmWork<C> work, srt;                       // srt: the sort-only work of a borrowed sort (a context's mW)
    typename C::Affine *d_bases = nullptr; fe *d_scalars = nullptr; uint32_t *d_pos = nullptr;
    bool borrowed = false;
    uint32_t n = 0, n_sort = 0;
    uint64_t nbt = 0, piece_bound = 0, entries = 0, pieces = 0;
    const MsmWork<C> &sorter() const { return borrowed ? srt : work; }
    uint32_t acc_form() const { return work.sh.quad_acc == 4 ? 4u : (work.sh.acc_pairs && C::WAVES_PER_SIMD_PAIRS != C::WAVES_PER_SIMD) ? 2u : 1u; }
    int alloc(const zk_msm_stage_in *in, uint32_t c, uint32_t plog) {
        n = in->n; borrowed = in->n_src != 0; n_sort = borrowed ? in->n_src : in->n;
        if (borrowed) {
            ZK_TRY(srt.alloc(n_sort, c, nullptr, nullptr, /*sort_only=*/true, 1, plog));
            if (in->shift_payload) srt.use_shift_payload();
            ZK_TRY(work.alloc(n, c, nullptr, &srt.sh, false, 1, plog));
        } else ZK_TRY(work.alloc(n, c, nullptr, nullptr, false, 1, plog));
        const MsmShape &sh = work.sh;
        nbt = (uint64_t)sh.nb << sh.plog;
        const uint64_t bound = (uint64_t)n_sort * sh.W, by_min = (bound + sh.chunk.seg_min - 1) / sh.chunk.seg_min;
        piece_bound = (sh.chunk.max_chunks(bound) < by_min ? sh.chunk.max_chunks(bound) : by_min) + nbt;     // <= the allocation: max_chunks(bound) + nbt + 1
        return ZK_OK;
    }
    int upload(const zk_msm_stage_in *in) {
        ZK_TRY(dev_upload(&d_bases, (const typename C::Affine *)in->bases, n));
        ZK_TRY(dev_upload(&d_scalars, (const fe *)in->scalars, n_sort));
        if (borrowed && in->pos) ZK_TRY(dev_upload(&d_pos, in->pos, n_sort));
        ZK_HIP(hipMemset(work.pieces, 0xff, sizeof(typename C::XYZZ) * piece_bound));
        return ZK_OK;
    }
    int launch(const zk_msm_stage_in *in, int canonical) {
        ZK_TRY(work.precompute(d_bases, n, nullptr));
        ZK_TRY((borrowed ? srt : work).enqueue_sort(d_scalars, nullptr, n_sort, canonical, nullptr));
        return work.enqueue_accumulate(borrowed ? srt.view_for(in->offset, d_pos) : work.view(), nullptr);
    }
    // off[], sorted[] and the chunk pieces; the entry count bounds the copies only after it was checked against the allocation
    int read_back(uint32_t *off, uint32_t *sorted, uint64_t *pieces_out) {
        ZK_HIP(hipMemcpy(off, sorter().off, sizeof(uint32_t) * (nbt + 1), hipMemcpyDeviceToHost));
        entries = off[nbt];
        if (entries > (uint64_t)n_sort * work.sh.W) return fail(ZK_ERR_INTERNAL, "stage probe: off[nb_total] exceeds n * W");
        if (entries) ZK_HIP(hipMemcpy(sorted, sorter().sorted, sizeof(uint32_t) * entries, hipMemcpyDeviceToHost));
        const uint32_t seg = work.sh.chunk.len((uint32_t)entries);
        pieces = entries ? (entries + seg - 1) / seg + nbt - 1 : 0;              // piece index = chunk + bucket
        if (pieces > piece_bound) return fail(ZK_ERR_INTERNAL, "stage probe: the chunk rule gives more pieces than its own bound");
        if (pieces) ZK_HIP(hipMemcpy(pieces_out, work.pieces, sizeof(typename C::XYZZ) * pieces, hipMemcpyDeviceToHost));
        return ZK_OK;
    }
    void release() {
        work.release(); srt.release();
        if (d_bases) hipFree(d_bases);
        if (d_scalars) hipFree(d_scalars);
        if (d_pos) hipFree(d_pos);
    }
};
static bool stage_in_ok(const zk_msm_stage_in *in, bool second) {
    if (!in->bases || !in->scalars || !in->n) return false;
    if (!in->n_src) return true;
    if (second || in->n > in->n_src) return false;
    if (!in->pos) return (uint64_t)in->offset + in->n <= in->n_src;
    for (uint32_t i = 0; i < in->n_src; i++) if (in->pos[i] != 0xffffffffu && in->pos[i] >= in->n) return false;
    return true;
}
template <class C>
static int msm_stage_probe(const zk_msm_stage_in *a, const zk_msm_stage_in *b, int canonical, uint32_t cbits, uint32_t plog, uint32_t tail_lanes, zk_msm_stage_out *o) {
    constexpr uint64_t AW = sizeof(typename C::Affine) / 8, XW = sizeof(typename C::XYZZ) / 8;
    typedef typename C::XYZZ X;
    StageSide<C> s[2];
    int rc = s[0].alloc(a, cbits, plog);
    if (rc == ZK_OK && b) rc = s[1].alloc(b, cbits, plog);
    const MsmShape &sh = s[0].work.sh;
    const uint64_t nbt = s[0].nbt, sets = sh.planes(), rowcol = ((1ull << sh.lo_bits()) + (1ull << sh.hi_bits())) * sets;
    if (rc == ZK_OK && b && (s[1].work.sh.nb != sh.nb || s[1].work.sh.plog != sh.plog)) rc = fail(ZK_ERR_ARG, "stage probe: the second MSM has other buckets");
    if (rc == ZK_OK && (o->table_cap < (uint64_t)sh.rows() * a->n * AW || o->off_cap < nbt + 1 || o->sorted_cap < (uint64_t)s[0].n_sort * sh.W ||
                        o->pieces_cap < s[0].piece_bound * XW || o->heavy_cap < nbt || o->bucket_cap < nbt * XW || o->partial_a_cap < rowcol * XW ||
                        o->partial_b_cap < sets * XW || o->result_cap < AW))
        rc = fail(ZK_ERR_ARG, "stage probe: an output capacity is too small");
    if (rc == ZK_OK && b && (o->off2_cap < nbt + 1 || o->sorted2_cap < (uint64_t)s[1].n_sort * sh.W || o->pieces2_cap < s[1].piece_bound * XW))
        rc = fail(ZK_ERR_ARG, "stage probe: an output capacity of the second MSM is too small");
    // ---- nothing was launched up to here
    auto run = [&]() -> int {
        ZK_TRY(s[0].upload(a));
        if (b) ZK_TRY(s[1].upload(b));
        MsmWork<C> &w = s[0].work;
        ZK_HIP(hipMemset(w.bucket, 0xff, sizeof(X) * nbt));
        ZK_HIP(hipMemset(w.partial_a, 0xff, sizeof(X) * rowcol));
        ZK_HIP(hipMemset(w.partial_b, 0xff, sizeof(X) * sets));
        if (b) ZK_TRY(s[1].launch(b, canonical));              // (its accumulation queued first, as the L-query's is before the H-query's tail)
        ZK_TRY(s[0].launch(a, canonical));
        ZK_TRY(w.enqueue_tail(nullptr, tail_lanes, b ? &s[1].work : nullptr));
        if (hipDeviceSynchronize() != hipSuccess) return fail(ZK_ERR_HIP, "MSM kernels failed");
        ZK_TRY(s[0].read_back(o->off, o->sorted, o->pieces));
        if (b) ZK_TRY(s[1].read_back(o->off2, o->sorted2, o->pieces2));
        uint32_t heavy = 0;
        ZK_HIP(hipMemcpy(&heavy, w.heavy_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
        const uint32_t lanes = tail_lanes == 4 || tail_lanes == 1 ? tail_lanes : sh.quad;
        const uint32_t v[32] = {sh.c, sh.W, sh.nb, sh.plog, (uint32_t)sets, sh.lo_bits(), sh.hi_bits(), sh.quad, sh.quad_acc, sh.acc_pairs ? 1u : 0u, s[0].acc_form(),
                                sh.rowcol_seg, sh.chunk.slots, sh.chunk.seg_min, sh.chunk.seg_max, (uint32_t)s[0].entries, MSM_HEAVY, MSM_TREE, lanes, sh.rows(),
                                (uint32_t)s[0].pieces, heavy, s[0].borrowed ? s[0].srt.sort_kbits : 0u, b ? 1u : 0u,
                                b ? s[1].work.sh.chunk.slots : 0u, b ? s[1].work.sh.chunk.seg_min : 0u, b ? s[1].work.sh.chunk.seg_max : 0u, (uint32_t)s[1].entries,
                                b ? s[1].acc_form() : 0u, (uint32_t)s[1].pieces, MSM_HEAVY_GRID, 0};
        memcpy(o->info, v, sizeof(v));
        if (heavy > nbt) return fail(ZK_ERR_INTERNAL, "stage probe: heavy_count exceeds the bucket count");
        if (heavy) ZK_HIP(hipMemcpy(o->heavy_list, w.heavy_list, sizeof(uint32_t) * heavy, hipMemcpyDeviceToHost));
        ZK_HIP(hipMemcpy(o->table, w.table, sizeof(typename C::Affine) * (size_t)sh.rows() * a->n, hipMemcpyDeviceToHost));
        ZK_HIP(hipMemcpy(o->bucket, w.bucket, sizeof(X) * nbt, hipMemcpyDeviceToHost));
        ZK_HIP(hipMemcpy(o->partial_a, w.partial_a, sizeof(X) * rowcol, hipMemcpyDeviceToHost));
        ZK_HIP(hipMemcpy(o->partial_b, w.partial_b, sizeof(X) * sets, hipMemcpyDeviceToHost));
        const typename C::Affine r = C::to_affine(w.finish());
        memcpy(o->result, &r, sizeof(r));
        return ZK_OK;
    };
    if (rc == ZK_OK) rc = run();
    s[0].release(); s[1].release();
    return rc;
}
}  // namespace
extern "C" int zk_msm_stage_probe(int g2, const zk_msm_stage_in *first, const zk_msm_stage_in *second, int canonical, uint32_t c, uint32_t plog,
                                  uint32_t tail_lanes, int device, zk_msm_stage_out *out) try {
    if (!first || !out || !out->table || !out->pieces || !out->bucket || !out->partial_a || !out->partial_b || !out->result || !out->off || !out->sorted || !out->heavy_list)
        return fail(ZK_ERR_ARG, "null argument");
    if (second && (!out->off2 || !out->sorted2 || !out->pieces2)) return fail(ZK_ERR_ARG, "null argument");
    if (plog > 7) return fail(ZK_ERR_ARG, "stage probe: plog above 7");
    if (!stage_in_ok(first, false) || (second && !stage_in_ok(second, true))) return fail(ZK_ERR_ARG, "stage probe: null bases or scalars, n = 0, or a borrowed sort whose offset / pos leave its n_src scalars or this MSM's n bases");
    ZK_TRY(use_device(device));
    return g2 ? msm_stage_probe<G2>(first, second, canonical, c, plog, tail_lanes, out) : msm_stage_probe<G1>(first, second, canonical, c, plog, tail_lanes, out);
} ZK_GUARD

// host-only: Fr elements between the canonical and the Montgomery (libff::Fp_model) representation, in place
extern "C" int zk_fr_convert(uint64_t *io, uint32_t n, int to_montgomery) try {
    if (n && !io) return fail(ZK_ERR_ARG, "null argument");
    for (uint32_t i = 0; i < n; i++) {
        fe v; memcpy(v.l, io + 4 * (size_t)i, 32);
        v = to_montgomery ? Fr::to_mont(v) : Fr::from_mont(v);
        memcpy(io + 4 * (size_t)i, v.l, 32);
    }
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_field_mul(const uint64_t *a, const uint64_t *b, uint64_t *out, uint32_t n, int field, int device) try {
    if (!a || !b || !out) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(device));
    fe *da = nullptr, *db = nullptr, *dout = nullptr;
    int rc = dev_upload(&da, (const fe *)a, n);
    if (rc == ZK_OK) rc = dev_upload(&db, (const fe *)b, n);
    if (rc == ZK_OK && hipMalloc(&dout, 32 * (size_t)(n ? n : 1)) != hipSuccess) rc = ZK_ERR_NOMEM;
    if (rc == ZK_OK && n) { ZK_LAUNCH(k_field_mul, zk_div_up(n, 256), 256, nullptr, (const fe *)da, (const fe *)db, dout, n, field); }
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "kernel failed");
    if (rc == ZK_OK && n && hipMemcpy(out, dout, 32 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = ZK_ERR_HIP;
    if (da) hipFree(da);
    if (db) hipFree(db);
    if (dout) hipFree(dout);
    return rc;
} ZK_GUARD

// ---- arithmetic probe (include/zkhip.h: test infrastructure).  One primitive of bn254.hpp per kernel instantiation, operands as given,
// raw result limbs back.  The field forms live here, the curve forms with the curve kernels (msm_impl.hpp: curve_probe), so that both pass
// through the same assembly post-pass as the kernels that prove.
namespace {
static ZK_HD fe2 probe_ld2(const fe *a) { fe2 r; r.c0 = a[0]; r.c1 = a[1]; return r; }
static ZK_HD void probe_st2(fe *o, const fe2 &v) { o[0] = v.c0; o[1] = v.c1; }
static ZK_HD fe probe_flag(bool b) { fe r = Fr::zero(); r.l[0] = b ? 1u : 0u; return r; }
#define ZK_PROBE_OP(NAME, NIN, NOUT, ...) \
    template <class F> struct NAME { static constexpr uint32_t IN = NIN, OUT = NOUT; static ZK_HD void run(const fe *a, fe *o) { __VA_ARGS__; } };
ZK_PROBE_OP(PrAdd, 2, 1, o[0] = F::add(a[0], a[1]))
ZK_PROBE_OP(PrSub, 2, 1, o[0] = F::sub(a[0], a[1]))
ZK_PROBE_OP(PrNeg, 1, 1, o[0] = F::neg(a[0]))
ZK_PROBE_OP(PrMul, 2, 1, o[0] = F::mul(a[0], a[1]))
ZK_PROBE_OP(PrReduceOnce, 1, 1, o[0] = F::reduce_once(a[0]))
ZK_PROBE_OP(PrCanon, 1, 1, o[0] = F::canon(a[0]))
ZK_PROBE_OP(PrLmul, 2, 1, o[0] = F::lmul(a[0], a[1]))
ZK_PROBE_OP(PrLsqr, 1, 1, o[0] = F::lsqr(a[0]))
ZK_PROBE_OP(PrLadd, 2, 1, o[0] = F::ladd(a[0], a[1]))
ZK_PROBE_OP(PrLsub, 2, 1, o[0] = F::lsub(a[0], a[1]))
ZK_PROBE_OP(PrLdbl, 1, 1, o[0] = F::ldbl(a[0]))
ZK_PROBE_OP(PrLneg, 1, 1, o[0] = F::lneg(a[0]))
ZK_PROBE_OP(PrLisZero, 1, 1, o[0] = probe_flag(F::lis_zero(a[0])))
ZK_PROBE_OP(PrLnegOp, 1, 1, o[0] = F::lneg_op(a[0]))
ZK_PROBE_OP(PrLmulNegOp, 2, 1, o[0] = F::lmul(a[0], F::lneg_op(a[1])))
ZK_PROBE_OP(PrLmul2, 4, 1, o[0] = F::lmul2(a[0], a[1], a[2], a[3]))
ZK_PROBE_OP(PrLmul2NegOp, 4, 1, o[0] = F::lmul2(a[0], a[1], a[2], F::lneg_op(a[3])))
ZK_PROBE_OP(PrLmul4, 8, 1, o[0] = F::lmul4(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]))
ZK_PROBE_OP(PrLmul4NegOp, 8, 1, o[0] = F::lmul4(a[0], a[1], a[2], F::lneg_op(a[3]), a[4], a[5], a[6], F::lneg_op(a[7])))
ZK_PROBE_OP(PrLmulX2, 4, 2, F::lmul_x2(a[0], a[1], a[2], a[3], o[0], o[1]))
ZK_PROBE_OP(PrLmul2X2, 8, 2, F::lmul2_x2(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], o[0], o[1]))
ZK_PROBE_OP(PrToMont, 1, 1, o[0] = F::to_mont(a[0]))
ZK_PROBE_OP(PrFromMont, 1, 1, o[0] = F::from_mont(a[0]))
ZK_PROBE_OP(PrInv, 1, 1, o[0] = F::inv(a[0]))
ZK_PROBE_OP(PrLsqrPair, 2, 2, F::lsqr_pair(a[0], a[1], o[0], o[1]))
// Fq2 (F = Fq2): elements are two words
ZK_PROBE_OP(Pr2Lmul, 4, 2, probe_st2(o, F::lmul(probe_ld2(a), probe_ld2(a + 2))))
ZK_PROBE_OP(Pr2Lsqr, 2, 2, probe_st2(o, F::lsqr(probe_ld2(a))))
ZK_PROBE_OP(Pr2Lmul2, 8, 2, probe_st2(o, F::lmul2(probe_ld2(a), probe_ld2(a + 2), probe_ld2(a + 4), probe_ld2(a + 6))))
ZK_PROBE_OP(Pr2Ladd, 4, 2, probe_st2(o, F::ladd(probe_ld2(a), probe_ld2(a + 2))))
ZK_PROBE_OP(Pr2Lsub, 4, 2, probe_st2(o, F::lsub(probe_ld2(a), probe_ld2(a + 2))))
ZK_PROBE_OP(Pr2LisZero, 2, 2, o[0] = probe_flag(F::lis_zero(probe_ld2(a))); o[1] = Fr::zero())
ZK_PROBE_OP(Pr2Ldbl, 2, 2, probe_st2(o, F::ldbl(probe_ld2(a))))
ZK_PROBE_OP(Pr2Lneg, 2, 2, probe_st2(o, F::lneg(probe_ld2(a))))
ZK_PROBE_OP(Pr2Canon, 2, 2, probe_st2(o, F::canon(probe_ld2(a))))
ZK_PROBE_OP(Pr2Inv, 2, 2, probe_st2(o, F::inv(F::canon(probe_ld2(a)))))
ZK_PROBE_OP(Pr2Eq, 4, 2, o[0] = probe_flag(F::eq(F::canon(probe_ld2(a)), F::canon(probe_ld2(a + 2)))); o[1] = Fr::zero())
#undef ZK_PROBE_OP

template <class Op>
__global__ void __launch_bounds__(64) k_arith_probe(const fe *__restrict__ in, fe *__restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe a[Op::IN], o[Op::OUT];
#pragma unroll
    for (uint32_t k = 0; k < Op::IN; k++) a[k] = in[(size_t)i * Op::IN + k];
    Op::run(a, o);
#pragma unroll
    for (uint32_t k = 0; k < Op::OUT; k++) out[(size_t)i * Op::OUT + k] = o[k];
}
template <class Op> int probe_launch(const fe *d_in, uint32_t n, fe *d_out) {
    ZK_LAUNCH((k_arith_probe<Op>), zk_div_up(n, 64), 64, nullptr, d_in, d_out, n);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}
// ldot6 takes its row from scalar registers: the row must be the same in every lane of a wave.  One case per block of 64 lanes, which all
// compute it (the row is read through a wave-uniform address, as the Poseidon kernels read theirs); lane 0 stores the result
template <class F>
__global__ void __launch_bounds__(64) k_arith_probe_dot6(const fe *__restrict__ in, fe *__restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    fe a[6];
#pragma unroll
    for (uint32_t k = 0; k < 6; k++) a[k] = in[(size_t)i * 12 + k];
    const fe o = F::ldot6(a, in + (size_t)i * 12 + 6);
    if (threadIdx.x == 0) out[i] = o;
}
template <class F> int probe_field(int idx, const fe *d_in, uint32_t n, fe *d_out) {
    if (idx == 25) {
        ZK_LAUNCH((k_arith_probe_dot6<F>), n, 64, nullptr, d_in, d_out, n);
        ZK_HIP(hipGetLastError());
        return ZK_OK;
    }
    switch (idx) {
    case 0: return probe_launch<PrAdd<F>>(d_in, n, d_out);
    case 1: return probe_launch<PrSub<F>>(d_in, n, d_out);
    case 2: return probe_launch<PrNeg<F>>(d_in, n, d_out);
    case 3: return probe_launch<PrMul<F>>(d_in, n, d_out);
    case 4: return probe_launch<PrReduceOnce<F>>(d_in, n, d_out);
    case 5: return probe_launch<PrCanon<F>>(d_in, n, d_out);
    case 6: return probe_launch<PrLmul<F>>(d_in, n, d_out);
    case 7: return probe_launch<PrLsqr<F>>(d_in, n, d_out);
    case 8: return probe_launch<PrLadd<F>>(d_in, n, d_out);
    case 9: return probe_launch<PrLsub<F>>(d_in, n, d_out);
    case 10: return probe_launch<PrLdbl<F>>(d_in, n, d_out);
    case 11: return probe_launch<PrLneg<F>>(d_in, n, d_out);
    case 12: return probe_launch<PrLisZero<F>>(d_in, n, d_out);
    case 13: return probe_launch<PrLnegOp<F>>(d_in, n, d_out);
    case 14: return probe_launch<PrLmulNegOp<F>>(d_in, n, d_out);
    case 15: return probe_launch<PrLmul2<F>>(d_in, n, d_out);
    case 16: return probe_launch<PrLmul2NegOp<F>>(d_in, n, d_out);
    case 17: return probe_launch<PrLmul4<F>>(d_in, n, d_out);
    case 18: return probe_launch<PrLmul4NegOp<F>>(d_in, n, d_out);
    case 19: return probe_launch<PrLmulX2<F>>(d_in, n, d_out);
    case 20: return probe_launch<PrLmul2X2<F>>(d_in, n, d_out);
    case 21: return probe_launch<PrToMont<F>>(d_in, n, d_out);
    case 22: return probe_launch<PrFromMont<F>>(d_in, n, d_out);
    case 23: return probe_launch<PrInv<F>>(d_in, n, d_out);
    case 26: return probe_launch<PrLsqrPair<F>>(d_in, n, d_out);
    }
    return fail(ZK_ERR_ARG, "unknown probe op");
}
int probe_fq2(int idx, const fe *d_in, uint32_t n, fe *d_out) {
    switch (idx) {
    case 0: return probe_launch<Pr2Lmul<Fq2>>(d_in, n, d_out);
    case 1: return probe_launch<Pr2Lsqr<Fq2>>(d_in, n, d_out);
    case 2: return probe_launch<Pr2Lmul2<Fq2>>(d_in, n, d_out);
    case 3: return probe_launch<Pr2Ladd<Fq2>>(d_in, n, d_out);
    case 4: return probe_launch<Pr2Lsub<Fq2>>(d_in, n, d_out);
    case 5: return probe_launch<Pr2LisZero<Fq2>>(d_in, n, d_out);
    case 6: return probe_launch<Pr2Ldbl<Fq2>>(d_in, n, d_out);
    case 7: return probe_launch<Pr2Lneg<Fq2>>(d_in, n, d_out);
    case 8: return probe_launch<Pr2Canon<Fq2>>(d_in, n, d_out);
    case 9: return probe_launch<Pr2Inv<Fq2>>(d_in, n, d_out);
    case 10: return probe_launch<Pr2Eq<Fq2>>(d_in, n, d_out);
    }
    return fail(ZK_ERR_ARG, "unknown probe op");
}
// words per case in and out; false for an op that does not exist
bool probe_shape(int op, uint32_t &in_words, uint32_t &out_words) {
    static const uint8_t field_in[27] = {2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 1, 1, 1, 2, 4, 4, 8, 8, 4, 8, 1, 1, 1, 0, 12, 2};   // (24 is not assigned)
    static const uint8_t fq2_in[11] = {4, 2, 8, 4, 4, 2, 2, 2, 2, 2, 4};
    static const uint8_t curve_in[10] = {2, 4, 6, 6, 8, 4, 8, 6, 4, 4}, curve_out[10] = {4, 4, 4, 4, 4, 16, 16, 16, 4, 2};   // in field elements
    if (op < 0) return false;
    const int dom = op & ~0xff, idx = op & 0xff;
    if (dom == ZK_PROBE_FR || dom == ZK_PROBE_FQ) {
        if (idx >= 27 || idx == 24) return false;
        in_words = field_in[idx]; out_words = idx == 19 || idx == 20 || idx == 26 ? 2 : 1;
    } else if (dom == ZK_PROBE_FQ2) {
        if (idx >= 11) return false;
        in_words = fq2_in[idx]; out_words = 2;
    } else if (dom == ZK_PROBE_G1 || dom == ZK_PROBE_G2) {
        if (idx >= 10) return false;
        const uint32_t ew = dom == ZK_PROBE_G2 ? 2 : 1;
        in_words = curve_in[idx] * ew; out_words = curve_out[idx] * ew;
    } else return false;
    return true;
}
}  // namespace

extern "C" int zk_arith_probe_shape(int op, uint32_t *in_words, uint32_t *out_words) try {
    if (!in_words || !out_words) return fail(ZK_ERR_ARG, "null argument");
    if (!probe_shape(op, *in_words, *out_words)) return fail(ZK_ERR_ARG, "unknown probe op");
    return ZK_OK;
} ZK_GUARD

extern "C" int zk_arith_probe(int op, const uint64_t *in, uint32_t n, uint64_t *out, int device) try {
    uint32_t wi = 0, wo = 0;
    if (!probe_shape(op, wi, wo)) return fail(ZK_ERR_ARG, "unknown probe op");
    if (n > (1u << 20)) return fail(ZK_ERR_ARG, "the probe takes at most 2^20 cases per call");
    if (n && (!in || !out)) return fail(ZK_ERR_ARG, "null argument");
    ZK_TRY(use_device(device));
    if (!n) return ZK_OK;
    fe *d_in = nullptr, *d_out = nullptr;
    int rc = dev_upload(&d_in, (const fe *)in, (size_t)n * wi);
    if (rc == ZK_OK && hipMalloc(&d_out, 32 * (size_t)n * wo) != hipSuccess) rc = fail(ZK_ERR_NOMEM, "out of device memory");
    if (rc == ZK_OK) {
        const int dom = op & ~0xff, idx = op & 0xff;
        if (dom == ZK_PROBE_FR) rc = probe_field<Fr>(idx, d_in, n, d_out);
        else if (dom == ZK_PROBE_FQ) rc = probe_field<Fq>(idx, d_in, n, d_out);
        else if (dom == ZK_PROBE_FQ2) rc = probe_fq2(idx, d_in, n, d_out);
        else if (dom == ZK_PROBE_G1) rc = curve_probe<G1>(idx, d_in, n, d_out);
        else rc = curve_probe<G2>(idx, d_in, n, d_out);
    }
    if (rc == ZK_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ZK_ERR_HIP, "probe kernel failed");
    if (rc == ZK_OK && hipMemcpy(out, d_out, 32 * (size_t)n * wo, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ZK_ERR_HIP, "copy from the device failed");
    if (d_in) hipFree(d_in);
    if (d_out) hipFree(d_out);
    return rc;
} ZK_GUARD
