// wplan_wide.hpp -- the lane-parallel ("wide") witness plan: a header of the zkhip.cpp unit (it uses that unit's fail(), fe / Fr and the
// zk_csr / zk_whint types of include/zkhip.h), included right before the zk_wplan entry points.
//
// The tape plan gives a witness ONE lane and walks the constraints as one dependent chain; a row of 63 general coefficients (a partial-round
// S-box input of Poseidon) is then 63 dependent products.  This plan gives a witness a GROUP of `lanes` lanes (4 .. 64; a wave holds
// 64 / lanes witnesses) and compiles the constraint system -- classified exactly as zk_wplan_create_hinted classifies it -- into a dataflow
// program of lane operations:
//     DOT    tmp = sum_{i < n} c_i val[s_i], n <= WW_T; the +-1 and constant-ONE shortcuts of the tape are kept.  A longer combination is
//            ceil(n / WW_T) chunk DOTs and a combining DOT over their temporaries (recursively).  IDENTICAL combinations (keyed by their
//            (column, coefficient) lists) are evaluated once while the temporary is live: the x^2 constraint of a Poseidon S-box has the same
//            row as A and B, the x^5 constraint has it again as B.
//     STEP   w[target] = (a b - c) inv, or for a constraint that introduces nothing bad += (a b - c != 0); a, b, c: a variable, a temporary,
//            a constant or empty
//     HINT   ZK_WHINT_BITS split over the lanes (each writes a contiguous run of the bits), ZK_WHINT_INV / ZK_WHINT_NONZERO one lane each
// Operations are levelled as soon as possible (level = 1 + the highest level among the inputs, supplied variables at 0); a level of more
// than `lanes` operations is split into passes of at most `lanes`; the program is the sequence of passes, laid out [pass][word][lane in
// group] so that a pass is one coalesced read.  Temporaries and recently produced variables live in LDS slots allocated HERE by liveness
// (the tape's compile-time-managed cache, now shared by the lanes of a group: 32 x lanes slots, the group's share of 64 KiB); variables
// also go to the witness row, and a variable whose slot was needed for something else is read back from there.
#pragma once
#include <array>
#include <map>
#include <set>

namespace {
constexpr uint32_t WW_T = 8;                                  // terms of one DOT
constexpr uint32_t WW_WORDS = 3 + 2 * WW_T;                   // words of an operation record
constexpr uint32_t WW_LDS_WORDS = 16384;                      // 64 KiB per workgroup, as the tape kernel: 2048 slots of 8 words
constexpr uint32_t WW_REUSE = 32;                             // a combination's temporary is reused by the next WW_REUSE constraints
constexpr uint32_t WW_NONE = 0xffffffffu;
enum { WW_NOP = 0, WW_DOT = 1, WW_STEP = 2, WW_HINT = 3 };
// record:  word 0   op | n << 4 | has_inverse << 8 | check << 9 | hint kind << 10 | A empty << 12 | B empty << 13 | C empty << 14 | (slot + 1) << 16
//          word 1   STEP: target variable                HINT: first variable this lane writes
//          word 2   STEP: index of 1 / C_{j,target}      HINT: number of variables this lane writes
//          words 3 + 2 i, 4 + 2 i   term i (DOT), operand a / b / c (STEP, i = 0 .. 2), source (HINT; word 4: the first bit this lane writes)
//   term.0  index | in_lds << 29 | kind << 30     kind 0: + v, 1: - v, 2: + coef v, 3: + coef (index = coefficient)      term.1  coefficient index
//           in_lds: index is an LDS slot of the group, else a variable of the witness row

// one shared, out-of-line product site: the eight term sites of a DOT and the STEP stay small.  (A function with its operands and result in
// registers -- the tape kernel's capturing lambda keeps them in scratch, a memory round trip per product.)
__device__ __attribute__((noinline)) fe ww_mul(fe a, fe b) { return Fr::mul(a, b); }

__global__ void __launch_bounds__(64)
k_witness_wide(const uint32_t *__restrict__ prog, uint32_t n_passes, const fe *__restrict__ coefs,
               fe *w, uint32_t stride, uint32_t k, uint32_t lanes_log2, uint32_t *__restrict__ violations) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[WW_LDS_WORDS];     // [group][slot][limb]
    const uint32_t lane = threadIdx.x, lanes = 1u << lanes_log2, li = lane & (lanes - 1), grp = lane >> lanes_log2;
    const uint32_t p = blockIdx.x * (64u >> lanes_log2) + grp;
    const bool live = p < k;
    fe *x = w + (size_t)(live ? p : 0) * stride;                 // (idle groups of the last wave shadow witness 0 and store nothing)
    uint32_t *slots = lds + (size_t)grp * (WW_LDS_WORDS >> (6 - lanes_log2));
    uint32_t bad = 0;
    auto slot_get = [&](uint32_t s) { fe v;
#pragma unroll
        for (int l = 0; l < 8; l++) v.l[l] = slots[s * 8 + l];
        return v; };
    auto slot_put = [&](uint32_t s, const fe &v) {
#pragma unroll
        for (int l = 0; l < 8; l++) slots[s * 8 + l] = v.l[l]; };
    // A variable read from the witness row was supplied by the caller or stored in an EARLIER pass by a lane of this workgroup: the
    // __syncthreads() that ends every pass orders that store before this load (workgroup scope), so a plain load sees it.
    auto fetch = [&](uint32_t t0) { const uint32_t idx = t0 & 0x0fffffffu;
        return (t0 >> 30) == 3 ? coefs[idx] : ((t0 >> 29) & 1u) ? slot_get(idx) : x[idx]; };
    uint32_t nx[WW_WORDS];                                       // the NEXT pass's record of this lane, requested one pass ahead
#pragma unroll
    for (uint32_t i = 0; i < WW_WORDS; i++) nx[i] = prog[(size_t)i * lanes + li];
    for (uint32_t pass = 0; pass < n_passes; pass++) {
        uint32_t rec[WW_WORDS];
#pragma unroll
        for (uint32_t i = 0; i < WW_WORDS; i++) rec[i] = nx[i];
        const uint32_t *nrec = prog + ((size_t)(pass + 1) * WW_WORDS) * lanes + li;      // (the program ends in an empty pass: reading ahead is safe)
#pragma unroll
        for (uint32_t i = 0; i < WW_WORDS; i++) nx[i] = nrec[(size_t)i * lanes];
        const uint32_t head = rec[0], op = head & 15u, dst1 = head >> 16;
        if (op == WW_DOT) {
            const uint32_t n = (head >> 4) & 15u;
            fe acc = Fr::zero();
#pragma unroll
            for (uint32_t i = 0; i < WW_T; i++) if (i < n) {
                const uint32_t t0 = rec[3 + 2 * i], kind = t0 >> 30;
                fe v = fetch(t0);
                if (kind == 2) v = ww_mul(coefs[rec[4 + 2 * i]], v);
                if (i == 0) acc = kind == 1 ? Fr::neg(v) : v;
                else acc = kind == 1 ? Fr::sub(acc, v) : Fr::add(acc, v);
            }
            if (dst1) slot_put(dst1 - 1, acc);
        } else if (op == WW_STEP) {
            const bool eA = (head >> 12) & 1u, eB = (head >> 13) & 1u, eC = (head >> 14) & 1u;
            fe v = Fr::zero();                                   // an empty sum is 0
            if (!(eA || eB)) v = ww_mul(fetch(rec[3]), fetch(rec[5]));
            if (!eC) v = Fr::sub(v, fetch(rec[7]));
            if ((head >> 9) & 1u) bad += live && !Fr::is_zero(v);
            else {
                if ((head >> 8) & 1u) v = ww_mul(coefs[rec[2]], v);
                if (live) x[rec[1]] = v;
                if (dst1) slot_put(dst1 - 1, v);
            }
        } else if (op == WW_HINT) {                               // see k_witness_tape for what the three kinds mean
            const uint32_t hk = (head >> 10) & 3u, first = rec[1], count = rec[2], bit0 = rec[4];
            const fe one = Fr::one();
            const fe s = fetch(rec[3]);
            if (hk == 0) {
                fe raw = Fr::zero(); raw.l[0] = 1;
                const fe v = ww_mul(raw, s);                     // out of the Montgomery form
                if (live) for (uint32_t i = 0; i < count; i++) {
                    const uint32_t b = bit0 + i;
                    uint32_t limb = 0;                           // (selected, not indexed: the limbs stay in registers)
#pragma unroll
                    for (uint32_t l = 0; l < 8; l++) limb = (b >> 5) == l ? v.l[l] : limb;
                    const bool set = (limb >> (b & 31)) & 1u;
                    fe o;
#pragma unroll
                    for (int l = 0; l < 8; l++) o.l[l] = set ? one.l[l] : 0u;
                    x[first + i] = o;
                }
            } else {
                fe r = Fr::inv(s);
                if (hk != 1) {
                    const bool nz = !Fr::is_zero(s);
#pragma unroll
                    for (int l = 0; l < 8; l++) r.l[l] = nz ? one.l[l] : 0u;
                }
                if (live) x[first] = r;
                if (dst1) slot_put(dst1 - 1, r);
            }
        }
        __syncthreads();
    }
    lds[lane] = bad;                                             // (after the last pass's barrier nothing reads the slots)
    __syncthreads();
    if (lane == 0) {
        uint32_t sum = 0;
        for (uint32_t i = 0; i < 64; i++) sum += lds[i];
        if (sum) atomicAdd(violations, sum);
    }
}

// ---------------------------------------------------------------- the plan compiler (host)
struct WwTerm { uint32_t val, kind, coef; };                      // val: a variable (<= V) or V + 1 + temporary; kind 3: no value, coef alone
struct WwOp {
    uint32_t op = WW_NOP, n = 0, flags = 0, level = 0, target = WW_NONE, inv = 0, out = WW_NONE, h_first = 0, h_count = 0, h_bit0 = 0;
    WwTerm t[WW_T];
};
struct WidePlanHost { std::vector<uint32_t> prog; std::vector<fe> coefs; zk_wplan_stats st; };

int wide_compile(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V, const uint8_t *known,
                 const zk_whint *hints, uint32_t n_hints, uint32_t lanes, WidePlanHost &out) {
    // ---- the classification of zk_wplan_create_hinted, restated: same order, same have[] bookkeeping, same refusals
    std::vector<uint8_t> have(known, known + (size_t)V + 1);
    have[0] = 1;
    std::vector<fe> &coefs = out.coefs;
    std::map<std::array<uint32_t, 8>, uint32_t> coef_map;
    auto coef_index = [&](const fe &c) -> uint32_t {
        std::array<uint32_t, 8> key; for (int i = 0; i < 8; i++) key[i] = c.l[i];
        auto it = coef_map.find(key);
        if (it != coef_map.end()) return it->second;
        coefs.push_back(c); coef_map[key] = (uint32_t)coefs.size() - 1; return (uint32_t)coefs.size() - 1;
    };
    const fe one = Fr::one(), minus_one = Fr::neg(one);
    std::vector<uint32_t> hint_of((size_t)V + 1, WW_NONE);
    std::vector<uint8_t> hint_done(n_hints, 0);
    for (uint32_t h = 0; h < n_hints; h++) {
        if (hints[h].kind != ZK_WHINT_BITS && hints[h].kind != ZK_WHINT_INV && hints[h].kind != ZK_WHINT_NONZERO) return fail(ZK_ERR_ARG, "witness plan: unknown hint kind");
        if (hints[h].kind != ZK_WHINT_BITS && hints[h].count != 1) return fail(ZK_ERR_ARG, "witness plan: ZK_WHINT_INV / ZK_WHINT_NONZERO define one variable (count = 1)");
        if (hints[h].src > V || hints[h].count == 0 || (uint64_t)hints[h].first + hints[h].count > (uint64_t)V + 1 || hints[h].first == 0) return fail(ZK_ERR_ARG, "witness plan: hint variables out of range");
        for (uint32_t i = 0; i < hints[h].count; i++) {
            if (have[hints[h].first + i] || hint_of[hints[h].first + i] != WW_NONE) return fail(ZK_ERR_ARG, "witness plan: a hint defines a variable that is supplied or defined twice");
            hint_of[hints[h].first + i] = h;
        }
    }
    std::vector<WwOp> ops;
    std::vector<uint32_t> lvl((size_t)V + 1, 0);                    // level of every value: variables, then temporaries
    uint32_t dots = 0, steps = 0, products = 0;
    char msg[200];
    auto try_hint = [&](uint32_t v) -> bool {
        const uint32_t h = v <= V ? hint_of[v] : WW_NONE;
        if (h == WW_NONE || hint_done[h] || !have[hints[h].src]) return false;
        const uint32_t level = lvl[hints[h].src] + 1, count = hints[h].count;
        const uint32_t parts = hints[h].kind == ZK_WHINT_BITS ? std::min(lanes, count) : 1u, per = (count + parts - 1) / parts;
        for (uint32_t b0 = 0; b0 < count; b0 += per) {
            WwOp o; o.op = WW_HINT; o.flags = (hints[h].kind - ZK_WHINT_BITS) << 10; o.level = level;
            o.n = 1; o.t[0] = {hints[h].src, 0u, 0u};
            o.h_first = hints[h].first + b0; o.h_count = std::min(per, count - b0); o.h_bit0 = b0;
            if (hints[h].kind != ZK_WHINT_BITS) o.out = hints[h].first;         // (the bits go to the witness row only)
            ops.push_back(o);
        }
        for (uint32_t i = 0; i < count; i++) { have[hints[h].first + i] = 1; lvl[hints[h].first + i] = level; }
        hint_done[h] = 1;
        return true;
    };
    auto new_dot = [&](const WwTerm *t, uint32_t n) -> uint32_t {    // one DOT of n <= WW_T terms; returns the temporary it produces
        WwOp o; o.op = WW_DOT; o.n = n;
        uint32_t level = 0;
        for (uint32_t i = 0; i < n; i++) { o.t[i] = t[i]; if (t[i].kind != 3) level = std::max(level, lvl[t[i].val]); products += t[i].kind == 2; }
        o.level = level + 1; o.out = (uint32_t)lvl.size();
        lvl.push_back(o.level);
        ops.push_back(o); dots++;
        return o.out;
    };
    std::map<std::vector<uint64_t>, std::pair<uint32_t, uint32_t>> rows;       // (column, coefficient) list -> its temporary, the constraint that made it
    for (uint32_t j = 0; j < nC; j++) {
        const zk_csr *M[2] = {A, B};
        for (int q = 0; q < 2; q++)
            for (uint32_t e = M[q]->row_ptr[j]; e < M[q]->row_ptr[j + 1]; e++) {
                if (M[q]->col[e] > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables");
                if (!have[M[q]->col[e]]) try_hint(M[q]->col[e]);
                if (!have[M[q]->col[e]]) { snprintf(msg, sizeof(msg), "constraint %u reads variable %u in %c before anything defines it: not in solved order", j, M[q]->col[e], q ? 'B' : 'A'); return fail(ZK_ERR_ARG, msg); }
            }
        uint32_t target = WW_NONE; fe tcoef = one;
        for (uint32_t e = C->row_ptr[j]; e < C->row_ptr[j + 1]; e++) {
            const uint32_t v = C->col[e];
            if (v > V) return fail(ZK_ERR_ARG, "CSR column index exceeds the number of variables");
            if (!have[v]) try_hint(v);
            if (have[v]) continue;
            if (target != WW_NONE) { snprintf(msg, sizeof(msg), "constraint %u introduces two new variables (%u and %u)", j, target, v); return fail(ZK_ERR_ARG, msg); }
            fe cf; memcpy(cf.l, C->coeff + 4 * (size_t)e, 32);
            if (Fr::is_zero(cf)) return fail(ZK_ERR_ARG, "zero coefficient on the variable a constraint introduces");
            target = v; tcoef = cf;
        }
        const bool has_inv = target != WW_NONE && !Fr::eq(tcoef, one);
        WwOp s; s.op = WW_STEP; s.target = target; s.n = 3;
        s.inv = has_inv ? coef_index(Fr::inv(tcoef)) : 0u;
        s.flags = (has_inv ? 1u << 8 : 0u) | (target == WW_NONE ? 1u << 9 : 0u);
        const zk_csr *Ms[3] = {A, B, C};
        uint32_t level = 0;
        for (int q = 0; q < 3; q++) {
            std::vector<WwTerm> terms;
            std::vector<uint64_t> key;
            for (uint32_t e = Ms[q]->row_ptr[j]; e < Ms[q]->row_ptr[j + 1]; e++) {
                const uint32_t col = Ms[q]->col[e];
                if (q == 2 && col == target) continue;
                fe cf; memcpy(cf.l, Ms[q]->coeff + 4 * (size_t)e, 32);
                if (Fr::is_zero(cf)) continue;
                uint32_t kind, ci = 0;
                if (col == 0) { kind = 3; ci = coef_index(cf); }
                else if (Fr::eq(cf, one)) kind = 0;
                else if (Fr::eq(cf, minus_one)) kind = 1;
                else { kind = 2; ci = coef_index(cf); }
                if (ci >= (1u << 28)) return fail(ZK_ERR_ARG, "witness plan: more than 2^28 distinct coefficients");
                terms.push_back({col, kind, ci});
                key.push_back((uint64_t)col << 32 | (uint64_t)kind << 28 | ci);
            }
            if (terms.empty()) { s.flags |= 1u << (12 + q); s.t[q] = {0u, 3u, 0u}; continue; }
            if (terms.size() == 1 && (terms[0].kind == 0 || terms[0].kind == 3)) {          // a lone variable or constant: no DOT
                s.t[q] = terms[0];
                if (terms[0].kind == 0) level = std::max(level, lvl[terms[0].val]);
                continue;
            }
            auto it = rows.find(key);
            uint32_t tmp;
            if (it != rows.end() && j - it->second.second <= WW_REUSE) tmp = it->second.first;
            else {
                while (terms.size() > WW_T) {                      // chunk DOTs, then a DOT over their temporaries
                    std::vector<WwTerm> up;
                    for (size_t at = 0; at < terms.size(); at += WW_T)
                        up.push_back({new_dot(terms.data() + at, (uint32_t)std::min<size_t>(WW_T, terms.size() - at)), 0u, 0u});
                    terms.swap(up);
                }
                tmp = new_dot(terms.data(), (uint32_t)terms.size());
                rows[key] = {tmp, j};
            }
            s.t[q] = {tmp, 0u, 0u};
            level = std::max(level, lvl[tmp]);
        }
        s.level = level + 1;
        if (!((s.flags >> 12) & 3u)) products++;
        products += has_inv;
        if (target != WW_NONE) { s.out = target; lvl[target] = s.level; have[target] = 1; }
        ops.push_back(s); steps++;
    }
    for (uint32_t v = 0; v <= V; v++) if (!have[v]) { snprintf(msg, sizeof(msg), "variable %u is neither supplied nor defined by a constraint", v); return fail(ZK_ERR_ARG, msg); }
    rows.clear();
    // The STEPs (and with them every variable and the number of levels) stay where "as soon as possible" puts them.  A DOT whose inputs are old
    // -- the chunks of a Poseidon row over the S-box outputs of ALL earlier rounds -- would be evaluated hundreds of levels before the
    // STEP that reads it, and its temporary would hold an LDS slot all that time (the preimage circuit at 4 lanes: > 128 live temporaries).
    // So a DOT sinks to the level right before its first reader: no STEP moves, no level is added.
    {
        std::vector<uint32_t> need(lvl.size(), WW_NONE);
        for (size_t i = ops.size(); i-- > 0;) {
            WwOp &o = ops[i];
            if (o.op == WW_DOT && need[o.out] != WW_NONE) { o.level = need[o.out]; lvl[o.out] = o.level; }
            if (o.op == WW_HINT) continue;
            for (uint32_t t = 0; t < o.n; t++)
                if (o.t[t].kind != 3 && !(o.op == WW_STEP && ((o.flags >> (12 + t)) & 1u)) && o.t[t].val > V) need[o.t[t].val] = std::min(need[o.t[t].val], o.level - 1);
        }
    }
    // ---- levels -> passes of at most `lanes` operations (within a level the kinds are kept together: less divergence inside a pass)
    uint32_t levels = 0;
    for (const WwOp &o : ops) levels = std::max(levels, o.level);
    std::vector<uint32_t> order(ops.size());
    for (uint32_t i = 0; i < ops.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (ops[a].level != ops[b].level) return ops[a].level < ops[b].level;
        if (ops[a].op != ops[b].op) return ops[a].op < ops[b].op;
        return ops[a].n > ops[b].n; });
    std::vector<uint32_t> pass_of(ops.size());
    uint32_t n_passes = 0, max_level_ops = 0;
    for (size_t i = 0, in_level = 0; i < order.size(); i++) {
        if (i && ops[order[i]].level != ops[order[i - 1]].level) { in_level = 0; n_passes++; }
        else if (i && in_level % lanes == 0) n_passes++;
        pass_of[order[i]] = n_passes;
        max_level_ops = std::max<uint32_t>(max_level_ops, (uint32_t)++in_level);
    }
    if (!order.empty()) n_passes++;
    // ---- in which passes every value is read
    const size_t n_vals = lvl.size();
    std::vector<uint32_t> use_ptr(n_vals + 1, 0), seen(n_vals, WW_NONE);
    auto for_sources = [&](const WwOp &o, auto &&f) { for (uint32_t i = 0; i < o.n; i++) if (o.t[i].kind != 3 && !(o.op == WW_STEP && ((o.flags >> (12 + i)) & 1u))) f(i); };
    for (uint32_t i : order) for_sources(ops[i], [&](uint32_t t) { const uint32_t v = ops[i].t[t].val; if (seen[v] != pass_of[i]) { seen[v] = pass_of[i]; use_ptr[v + 1]++; } });
    for (size_t v = 0; v < n_vals; v++) use_ptr[v + 1] += use_ptr[v];
    std::vector<uint32_t> uses(use_ptr[n_vals]), fill(use_ptr.begin(), use_ptr.end() - 1);
    std::fill(seen.begin(), seen.end(), WW_NONE);
    for (uint32_t i : order) for_sources(ops[i], [&](uint32_t t) { const uint32_t v = ops[i].t[t].val; if (seen[v] != pass_of[i]) { seen[v] = pass_of[i]; uses[fill[v]++] = pass_of[i]; } });
    // ---- LDS slots by liveness, and the records
    const uint32_t n_slots = 32 * lanes;
    std::vector<uint32_t> free_slots(n_slots);
    for (uint32_t i = 0; i < n_slots; i++) free_slots[i] = n_slots - 1 - i;
    std::vector<uint32_t> slot_of(n_vals, WW_NONE), use_pos(use_ptr.begin(), use_ptr.end() - 1), last_read(n_vals, WW_NONE), def_pass(n_vals, WW_NONE);
    std::vector<uint32_t> rel_head((size_t)n_passes + 2, WW_NONE), rel_next(n_vals, WW_NONE);
    std::set<std::pair<uint32_t, uint32_t>> cached;                 // variables that hold a slot and are read again: (pass of the next read, variable)
    uint32_t in_use = 0, peak = 0, live_tmps = 0;
    out.prog.assign(((size_t)n_passes + 1) * WW_WORDS * lanes, 0u);  // (one empty pass at the end: the kernel reads one pass ahead)
    size_t at = 0;
    for (uint32_t p = 0; p < n_passes; p++) {
        for (uint32_t v = rel_head[p]; v != WW_NONE; v = rel_next[v])
            if (slot_of[v] != WW_NONE) { free_slots.push_back(slot_of[v]); slot_of[v] = WW_NONE; in_use--; live_tmps -= v > V; }
        const size_t begin = at;
        while (at < order.size() && pass_of[order[at]] == p) at++;
        auto word = [&](size_t o, uint32_t wd) -> uint32_t & { return out.prog[((size_t)p * WW_WORDS + wd) * lanes + (o - begin)]; };
        for (size_t o = begin; o < at; o++) {                       // what this pass reads, and from where
            const WwOp &op = ops[order[o]];
            word(o, 0) = op.op | op.n << 4 | op.flags;
            if (op.op == WW_STEP) { word(o, 1) = op.target; word(o, 2) = op.inv; }
            if (op.op == WW_HINT) { word(o, 1) = op.h_first; word(o, 2) = op.h_count; word(o, 4) = op.h_bit0; }
            for (uint32_t i = 0; i < op.n; i++) {
                const WwTerm &t = op.t[i];
                if (op.op == WW_STEP && ((op.flags >> (12 + i)) & 1u)) continue;
                if (t.kind == 3) { word(o, 3 + 2 * i) = 3u << 30 | t.coef; continue; }
                const uint32_t v = t.val;
                if (slot_of[v] == WW_NONE && v > V) return fail(ZK_ERR_INTERNAL, "witness plan (wide): a temporary lost its slot");
                word(o, 3 + 2 * i) = t.kind << 30 | (slot_of[v] != WW_NONE ? 1u << 29 | slot_of[v] : v);
                if (op.op == WW_DOT) word(o, 4 + 2 * i) = t.coef;
                if (last_read[v] == p) continue;
                last_read[v] = p;
                const bool holds = slot_of[v] != WW_NONE && v <= V;
                if (holds) cached.erase({uses[use_pos[v]], v});
                if (++use_pos[v] < use_ptr[v + 1]) { if (holds) cached.insert({uses[use_pos[v]], v}); }
                else { rel_next[v] = rel_head[p + 1]; rel_head[p + 1] = v; }     // the last read: the slot is free from the next pass on
            }
        }
        uint32_t tmps_here = 0;
        for (size_t o = begin; o < at; o++) tmps_here += ops[order[o]].out != WW_NONE && ops[order[o]].out > V;
        for (size_t o = begin; o < at; o++) {                       // what this pass produces: temporaries must get a slot, variables get one if it pays
            const WwOp &op = ops[order[o]];
            const uint32_t v = op.out;
            if (v == WW_NONE) continue;
            def_pass[v] = p;
            if (use_ptr[v] == use_ptr[v + 1]) continue;             // never read again
            const bool tmp = v > V;
            if (free_slots.empty()) {
                // take the slot of the variable whose next read is farthest away (it is read from the witness row from then on); not one
                // that this pass reads or has just produced: its slot is in use until the barrier
                auto victim = cached.end();
                for (auto it = cached.rbegin(); it != cached.rend(); ++it)
                    if (last_read[it->second] != p && def_pass[it->second] != p) { victim = std::prev(it.base()); break; }
                if (!tmp && (victim == cached.end() || victim->first <= uses[use_ptr[v]])) continue;
                if (victim == cached.end()) {
                    snprintf(msg, sizeof(msg), "witness plan (wide): level %u needs %u live LDS slots (%u of them temporaries), a group of %u lanes has %u: use more lanes", op.level, in_use + tmps_here, live_tmps + tmps_here, lanes, n_slots);
                    return fail(ZK_ERR_ARG, msg);
                }
                free_slots.push_back(slot_of[victim->second]); slot_of[victim->second] = WW_NONE; in_use--;
                cached.erase(victim);
            }
            slot_of[v] = free_slots.back(); free_slots.pop_back();
            peak = std::max(peak, ++in_use); live_tmps += tmp;
            if (tmp) tmps_here--;
            else cached.insert({uses[use_ptr[v]], v});
            word(o, 0) |= (slot_of[v] + 1) << 16;
        }
    }
    zk_wplan_stats &st = out.st;
    st.kind = 1; st.lanes = lanes; st.records_or_passes = n_passes; st.levels = levels; st.ops = (uint32_t)ops.size(); st.dots = dots; st.steps = steps;
    st.max_level_ops = max_level_ops; st.lds_slots = peak; st.products = products;
    if (coefs.empty()) coefs.push_back(one);
    return ZK_OK;
}
}  // namespace
