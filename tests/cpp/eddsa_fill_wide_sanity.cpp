// Host-only sanity of zk_eddsa_fill_witnesses_wide (csrc/jubjub.cpp, jubjub.hpp k_eddsa_fill_wide) for a sanitizer build: a stand-alone program
// over the CPU stand-in build of the library (-DZK_EMUL), where the 128 or 256 threads of a workgroup run as fibers that yield at the barriers.
// It drives the refusals, malformed items alone in their workgroup, and fills one row with 2 and with 4 lanes, which must leave the bytes that
// one lane leaves.  Build (from the repository root) and run on a development machine, never on a GPU and never loaded into Python; as in
// eddsa_fill_sanity.cpp only the unit under test and this driver are instrumented.  The fibers' stacks hold the instrumented frames: 4 MiB each.
//   F="-O1 -g -std=c++17 -DZK_EMUL -DZK_EMUL_FIBER_STACK=4194304 -Itests/emul -fno-omit-frame-pointer -x c++"; S="-fsanitize=address,undefined"; O=$(mktemp -d)
//   for u in zkhip msm_g1 msm_g2 verify pkjson; do g++ $F -c ethsnarks_amd/csrc/$u.cpp -o $O/$u.o & done
//   g++ $F $S -c ethsnarks_amd/csrc/jubjub.cpp -o $O/jubjub.o & g++ $F $S -c tests/cpp/eddsa_fill_wide_sanity.cpp -o $O/driver.o & wait
//   g++ $S $O/*.o -lpthread -o eddsa_fill_wide_sanity && ./eddsa_fill_wide_sanity
// layout1() is that of eddsa_fill_sanity.cpp; tests/test_jubjub_gadgets.py::test_circuit_shape pins the same tuple.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/zkhip.h"

extern "C" uint64_t zk_emul_guard_violations(void);               // of the CPU stand-in (tests/emul/hip_emul.h)

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { failures++; fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, zk_last_error()); } } while (0)

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
    std::vector<uint64_t> start(4 * (elems + guard) * 2), got(start.size()), one_lane(start.size());
    for (size_t i = 0; i < start.size(); i++) start[i] = 7 + i;
    void *d = nullptr;
    EXPECT(zk_dev_alloc(start.size() * 8, 0, &d) == ZK_OK);
    EXPECT(zk_dev_upload(d, start.data(), start.size() * 8) == ZK_OK);
    uint8_t verdict = 9;
    auto untouched = [&]() { EXPECT(zk_dev_download(got.data(), d, got.size() * 8) == ZK_OK); return verdict == 9 && got == start; };

    const uint32_t bad_lanes[3] = {0, 3, 8};
    for (uint32_t lanes : bad_lanes) EXPECT(zk_eddsa_fill_witnesses_wide(v, G, G, s, msg, 1, d, elems + guard, &good, &verdict, lanes) == ZK_ERR_ARG && untouched());
    const uint32_t wide[2] = {2, 4};
    for (uint32_t lanes : wide) {
        EXPECT(zk_eddsa_fill_witnesses_wide(pure, G, G, s, msg, 1, d, elems + guard, &good, &verdict, lanes) == ZK_ERR_ARG && untouched());
        EXPECT(zk_eddsa_fill_witnesses_wide(v, G, G, s, msg, 1, d, elems - 1, &good, &verdict, lanes) == ZK_ERR_ARG && untouched());
        EXPECT(zk_eddsa_fill_witnesses_wide(v, nullptr, G, s, msg, 1, d, elems, &good, &verdict, lanes) == ZK_ERR_ARG && untouched());
        EXPECT(zk_eddsa_fill_witnesses_wide(v, G, G, s, msg, 1, d, elems, nullptr, &verdict, lanes) == ZK_ERR_ARG && untouched());
        // malformed items, alone in their workgroup: verdict 0, no write, and every barrier passed
        EXPECT(zk_eddsa_fill_witnesses_wide(v, off, G, s, msg, 1, d, elems + guard, &good, &verdict, lanes) == ZK_OK && verdict == 0);
        verdict = 9; EXPECT(untouched());
        EXPECT(zk_eddsa_fill_witnesses_wide(v, G, G, big_s, msg, 1, d, elems + guard, &good, &verdict, lanes) == ZK_OK && verdict == 0);
        verdict = 9; EXPECT(untouched());
    }
    // a well-formed wrong signature: one lane first, then 2 and 4 lanes over a fresh buffer -- the same bytes, guards and second row included
    EXPECT(zk_eddsa_fill_witnesses_wide(v, G, G, s, msg, 1, d, elems + guard, &good, &verdict, 1) == ZK_OK && verdict == 0);
    EXPECT(zk_dev_download(one_lane.data(), d, one_lane.size() * 8) == ZK_OK);
    size_t changed = 0;
    for (size_t e = 0; e < elems; e++) changed += memcmp(&one_lane[4 * e], &start[4 * e], 32) != 0;
    EXPECT(changed == elems);
    EXPECT(memcmp(&one_lane[4 * elems], &start[4 * elems], (start.size() - 4 * elems) * 8) == 0);
    for (uint32_t lanes : wide) {
        EXPECT(zk_dev_upload(d, start.data(), start.size() * 8) == ZK_OK);
        verdict = 9;
        EXPECT(zk_eddsa_fill_witnesses_wide(v, G, G, s, msg, 1, d, elems + guard, &good, &verdict, lanes) == ZK_OK && verdict == 0);
        EXPECT(zk_dev_download(got.data(), d, got.size() * 8) == ZK_OK);
        EXPECT(got == one_lane);
    }
    EXPECT(zk_emul_guard_violations() == 0);
    zk_dev_free(d);
    zk_eddsa_free(v); zk_eddsa_free(pure);
    printf(failures ? "%d FAILURES\n" : "eddsa_fill_wide_sanity: ok\n", failures);
    return failures != 0;
}
