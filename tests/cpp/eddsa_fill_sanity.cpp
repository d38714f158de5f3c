// Host-only sanity of zk_eddsa_fill_witnesses (csrc/jubjub.cpp, jubjub.hpp) for a sanitizer build: a stand-alone program over the CPU stand-in
// build of the library (-DZK_EMUL).  It drives the argument checks and the layout validation, then fills one row and looks at its ends.
// Build (from the repository root) and run on a development machine, never on a GPU and never loaded into Python.  Only the unit under test
// (jubjub.cpp) and this driver are instrumented; the other units are compiled plainly and side by side, which keeps the build to about 7 minutes
// on 8 cores (msm_g2.cpp is the longest; jubjub.cpp under the sanitizers takes about 2).  Instrumenting every unit takes several times as long:
//   F="-O1 -g -std=c++17 -DZK_EMUL -Itests/emul -fno-omit-frame-pointer -x c++"; S="-fsanitize=address,undefined"; O=$(mktemp -d)
//   for u in zkhip msm_g1 msm_g2 verify pkjson; do g++ $F -c ethsnarks_amd/csrc/$u.cpp -o $O/$u.o & done
//   g++ $F $S -c ethsnarks_amd/csrc/jubjub.cpp -o $O/jubjub.o & g++ $F $S -c tests/cpp/eddsa_fill_sanity.cpp -o $O/driver.o & wait
//   g++ $S $O/*.o -lpthread -o eddsa_fill_sanity && ./eddsa_fill_sanity
// layout1() restates the offsets of the front end's layout; tests/test_jubjub_gadgets.py::test_circuit_shape pins the same tuple, so a change of
// the row fails there first and this file follows.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/zkhip.h"

extern "C" uint64_t zk_emul_guard_violations(void);               // of the CPU stand-in (tests/emul/hip_emul.h)

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { failures++; fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, zk_last_error()); } } while (0)

// the layout of eddsa_mimc_circuit(msg_len = 1) (ethsnarks_amd/jubjub_gadgets.py; tests/test_jubjub_gadgets.py pins the same tuple)
static zk_eddsa_layout layout1() {
    zk_eddsa_layout l;
    l.msg_len = 1; l.n_vars = 7907; l.ax_var = 1; l.msg_var0 = 3; l.rx_var = 4; l.s_bit0 = 6; l.iv_var = 260; l.validator_var0 = 261; l.window_var0 = 283;
    l.fixed_adder_var0 = 537; l.mimc_var0 = 1419; l.t_bit0 = 3244; l.t_range_var0 = 4005; l.cond0_var = 4104; l.doubler_var0 = 4106; l.cond_var0 = 4112;
    l.adder_var0 = 4114; l.step_stride = 15; l.last_adder_var0 = 7901;
    return l;
}

int main() {
    static const uint64_t G[8] = {0x79f2349047d5c157ull, 0xc88fee14d607cbe7ull, 0x6e35bc47bd9afe6cull, 0x2491aba8d3a191a7ull,
                                  0x348dd8f7f99152d7ull, 0xf9a9d4ed0cb0c1d1ull, 0x18dbddfd24c35583ull, 0x2e07297f8d3c3d78ull};   // the generator
    const uint64_t s[4] = {5, 0, 0, 0}, msg[4] = {7, 0, 0, 0}, off[8] = {1, 0, 0, 0, 1, 0, 0, 0}, big_s[4] = {0, 0, 0, 1ull << 62};
    const zk_eddsa_layout good = layout1();
    const uint64_t elems = good.n_vars + 1, guard = 3;
    zk_eddsa *v = nullptr, *pure = nullptr;
    EXPECT(zk_eddsa_create(ZK_EDDSA_MIMC, nullptr, 1, 0, &v) == ZK_OK);
    EXPECT(zk_eddsa_create(ZK_EDDSA_PURE, nullptr, 1, 0, &pure) == ZK_OK);
    std::vector<uint64_t> start(4 * (elems + guard) * 2), got(start.size());
    for (size_t i = 0; i < start.size(); i++) start[i] = 7 + i;
    void *d = nullptr;
    EXPECT(zk_dev_alloc(start.size() * 8, 0, &d) == ZK_OK);
    EXPECT(zk_dev_upload(d, start.data(), start.size() * 8) == ZK_OK);
    uint8_t verdict = 9;
    auto untouched = [&]() { EXPECT(zk_dev_download(got.data(), d, got.size() * 8) == ZK_OK); return verdict == 9 && got == start; };

    EXPECT(zk_eddsa_fill_witnesses(pure, G, G, s, msg, 1, d, elems + guard, &good, &verdict) == ZK_ERR_ARG && untouched());
    EXPECT(zk_eddsa_fill_witnesses(v, G, G, s, msg, 1, d, elems - 1, &good, &verdict) == ZK_ERR_ARG && untouched());
    EXPECT(zk_eddsa_fill_witnesses(v, nullptr, G, s, msg, 1, d, elems, &good, &verdict) == ZK_ERR_ARG && untouched());
    EXPECT(zk_eddsa_fill_witnesses(v, G, G, s, msg, 1, d, elems, nullptr, &verdict) == ZK_ERR_ARG && untouched());
    const uint32_t n_fields = sizeof(zk_eddsa_layout) / sizeof(uint32_t);
    for (uint32_t f = 0; f < n_fields; f++) {                      // every field pushed out of a row of exactly n_vars + 1 elements, and to 0
        const uint32_t bad[4] = {0xFFFFFFFFu, 0, (uint32_t)elems, 0x80000000u};
        for (uint32_t b : bad) {
            zk_eddsa_layout l = good;
            uint32_t w[n_fields];
            memcpy(w, &l, sizeof(l));
            if (w[f] == b) continue;
            w[f] = b;
            memcpy(&l, w, sizeof(l));
            EXPECT(zk_eddsa_fill_witnesses(v, G, G, s, msg, 1, d, elems, &l, &verdict) == ZK_ERR_ARG && untouched());
        }
    }
    // malformed items: verdict 0 and no write
    EXPECT(zk_eddsa_fill_witnesses(v, off, G, s, msg, 1, d, elems + guard, &good, &verdict) == ZK_OK && verdict == 0);
    verdict = 9; EXPECT(untouched());
    EXPECT(zk_eddsa_fill_witnesses(v, G, G, big_s, msg, 1, d, elems + guard, &good, &verdict) == ZK_OK && verdict == 0);
    verdict = 9; EXPECT(untouched());
    // a well-formed wrong signature: the whole row, the guard elements and the second row untouched
    EXPECT(zk_eddsa_fill_witnesses(v, G, G, s, msg, 1, d, elems + guard, &good, &verdict) == ZK_OK && verdict == 0);
    EXPECT(zk_dev_download(got.data(), d, got.size() * 8) == ZK_OK);
    uint64_t one[4] = {1, 0, 0, 0};
    EXPECT(zk_fr_convert(one, 1, 1) == ZK_OK);
    EXPECT(memcmp(got.data(), one, 32) == 0);
    size_t changed = 0;
    for (size_t e = 0; e < elems; e++) changed += memcmp(&got[4 * e], &start[4 * e], 32) != 0;
    EXPECT(changed == elems);
    EXPECT(memcmp(&got[4 * elems], &start[4 * elems], (start.size() - 4 * elems) * 8) == 0);
    EXPECT(zk_emul_guard_violations() == 0);
    zk_dev_free(d);
    zk_eddsa_free(v); zk_eddsa_free(pure);
    printf(failures ? "%d FAILURES\n" : "eddsa_fill_sanity: ok\n", failures);
    return failures != 0;
}
