// Host-only sanity of the wide witness plan's compiler (csrc/wplan_wide.hpp) for a sanitizer build: a stand-alone program over the CPU
// stand-in build of the library (-DZK_EMUL), the hand-made systems of tests/test_wplan_wide_emul.py.  Build (from the repository root):
//   g++ -O1 -g -std=c++17 -DZK_EMUL -DZK_EMUL_FIBER_STACK=4194304 -Itests/emul -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ \
//       tests/cpp/wplan_wide_sanity.cpp ethsnarks_amd/csrc/{zkhip,msm_g1,msm_g2,verify,pkjson}.cpp -lpthread -o wplan_wide_sanity
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/zkhip.h"

struct Sys {
    std::vector<uint32_t> ptr[3], col[3];
    std::vector<uint64_t> coef[3];
    uint32_t V = 0;
    zk_csr m[3];
    void row(int q, const std::vector<std::pair<uint32_t, uint64_t>> &terms, const uint64_t one_mont[4]) {
        if (ptr[q].empty()) ptr[q].push_back(0);
        for (auto &t : terms) {
            col[q].push_back(t.first);
            uint64_t canon[4] = {t.second, 0, 0, 0}, mont[4];
            if (t.second == 1) memcpy(mont, one_mont, 32);
            else if (memcpy(mont, canon, 32), zk_fr_convert(mont, 1, 1) != 0) { fprintf(stderr, "zk_fr_convert: %s\n", zk_last_error()); exit(2); }
            coef[q].insert(coef[q].end(), mont, mont + 4);
        }
        ptr[q].push_back((uint32_t)col[q].size());
    }
    void finish() { for (int q = 0; q < 3; q++) { m[q].n_rows = (uint32_t)ptr[q].size() - 1; m[q].row_ptr = ptr[q].data(); m[q].col = col[q].data(); m[q].coeff = coef[q].data(); } }
};

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { failures++; fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, zk_last_error()); } } while (0)

static zk_wplan_stats plan_and_solve(Sys &s, const std::vector<uint32_t> &supplied, uint32_t lanes, uint32_t k, int expect_rc = 0) {
    s.finish();
    std::vector<uint8_t> known(s.V + 1, 0);
    for (uint32_t v : supplied) known[v] = 1;
    zk_wplan *tape = nullptr, *wide = nullptr;
    zk_wplan_stats st; memset(&st, 0, sizeof(st));
    int rc = zk_wplan_create_wide(&s.m[0], &s.m[1], &s.m[2], s.m[0].n_rows, s.V, known.data(), nullptr, 0, lanes, 0, &wide);
    EXPECT(rc == expect_rc);
    if (rc != 0) return st;
    EXPECT(zk_wplan_create(&s.m[0], &s.m[1], &s.m[2], s.m[0].n_rows, s.V, known.data(), 0, &tape) == 0);
    EXPECT(zk_wplan_info(wide, &st) == 0);
    // k rows (variable v of row p = 3 v + p + 1, Montgomery form of small numbers is not needed: any field elements do) and a sentinel row
    const size_t row = 4 * (size_t)(s.V + 1);
    std::vector<uint64_t> start(row * (k + 1), 0), got[2];
    for (uint32_t p = 0; p < k; p++) for (uint32_t v : supplied) {
        uint64_t canon[4] = {v == 0 ? 1 : 3ull * v + p + 1, 0, 0, 0};
        memcpy(&start[row * p + 4 * v], canon, 32);
        EXPECT(zk_fr_convert(&start[row * p + 4 * v], 1, 1) == 0);
    }
    for (size_t i = 0; i < row; i++) start[row * k + i] = 7 + i;
    zk_wplan *plans[2] = {tape, wide};
    uint32_t bad[2] = {99, 99};
    for (int i = 0; i < 2; i++) {
        void *d = nullptr;
        EXPECT(zk_dev_alloc(start.size() * 8, 0, &d) == 0);
        EXPECT(zk_dev_upload(d, start.data(), start.size() * 8) == 0);
        EXPECT(zk_wplan_solve(plans[i], d, k, &bad[i]) == 0);
        got[i].resize(start.size());
        EXPECT(zk_dev_download(got[i].data(), d, start.size() * 8) == 0);
        EXPECT(zk_dev_free(d) == 0);
    }
    EXPECT(bad[0] == bad[1]);
    EXPECT(got[0] == got[1]);
    EXPECT(memcmp(&got[1][row * k], &start[row * k], row * 8) == 0);
    zk_wplan_free(tape); zk_wplan_free(wide);
    return st;
}

int main() {
    uint64_t one[4] = {1, 0, 0, 0};
    if (zk_fr_convert(one, 1, 1) != 0) { fprintf(stderr, "zk_fr_convert: %s\n", zk_last_error()); return 2; }
    const uint32_t n = 40;
    {   // independent constraints w[n + i] = w[i] w[i]
        Sys s; s.V = 2 * n;
        std::vector<uint32_t> sup = {0};
        for (uint32_t i = 1; i <= n; i++) { s.row(0, {{i, 1}}, one); s.row(1, {{i, 1}}, one); s.row(2, {{n + i, 1}}, one); sup.push_back(i); }
        zk_wplan_stats st = plan_and_solve(s, sup, 16, 5);
        EXPECT(st.levels == 1 && st.records_or_passes == 3 && st.steps == 40);
    }
    {   // a chain w[i + 1] = w[i] w[i]
        Sys s; s.V = n + 1;
        for (uint32_t i = 1; i <= n; i++) { s.row(0, {{i, 1}}, one); s.row(1, {{i, 1}}, one); s.row(2, {{i + 1, 1}}, one); }
        zk_wplan_stats st = plan_and_solve(s, {0, 1}, 4, 17);
        EXPECT(st.levels == 40 && st.records_or_passes == 40);
    }
    for (int same = 0; same < 2; same++) {   // a 64-term row with general coefficients, as A alone and as A and B
        Sys s; s.V = 65;
        std::vector<std::pair<uint32_t, uint64_t>> row;
        std::vector<uint32_t> sup = {0};
        for (uint32_t i = 1; i <= 64; i++) { row.push_back({i, i + 2}); sup.push_back(i); }
        s.row(0, row, one);
        if (same) s.row(1, row, one); else s.row(1, {{0, 1}}, one);
        s.row(2, {{65, 1}}, one);
        zk_wplan_stats st = plan_and_solve(s, sup, 64, 2);
        EXPECT(st.dots == 9 && st.levels == 3);
    }
    {   // 200 long rows whose readers wait for one late variable: refused at 4 lanes (128 slots), accepted at 16; a check row at the end
        Sys s; const uint32_t m = 200, chain = 4, late = chain + 1, base = chain + 2; s.V = base + 16 + m - 1;
        std::vector<uint32_t> sup = {0, 1};
        for (uint32_t i = 0; i < 16; i++) sup.push_back(base + i);
        for (uint32_t i = 1; i <= chain; i++) { s.row(0, {{i, 1}}, one); s.row(1, {{i, 1}}, one); s.row(2, {{i + 1, 1}}, one); }
        for (uint32_t i = 0; i < m; i++) {
            std::vector<std::pair<uint32_t, uint64_t>> row;
            for (uint32_t t = 0; t < 9; t++) row.push_back({base + (i + t) % 16, 3 + i + t});
            s.row(0, row, one); s.row(1, {{late, 1}}, one); s.row(2, {{base + 16 + i, 1}}, one);
        }
        s.row(0, {{1, 1}}, one); s.row(1, {{1, 1}}, one); s.row(2, {{3, 1}}, one);           // w1 w1 = w3: false, counted by both plans
        plan_and_solve(s, sup, 4, 1, 1);
        zk_wplan_stats st = plan_and_solve(s, sup, 16, 6);
        EXPECT(st.kind == 1 && st.lds_slots >= 200);
    }
    for (uint32_t lanes : {0u, 2u, 3u, 128u}) {
        Sys s; s.V = 2;
        s.row(0, {{1, 1}}, one); s.row(1, {{1, 1}}, one); s.row(2, {{2, 1}}, one);
        plan_and_solve(s, {0, 1}, lanes, 1, 1);
    }
    printf(failures ? "%d FAILURES\n" : "wplan_wide_sanity: ok\n", failures);
    return failures ? 1 : 0;
}
