/*
 * Stand-alone sanitizer program of the replace emulation — TEST TOOLING ONLY (tests/test_emu_replace.py compiles it with g++ -fsanitize=address,undefined and runs
 * it as a child process).  It builds logs of elements of 0, 1, 2 and 3 code units itself — chains of n x "a" for n around the tile of 64 hits, random mixes, a
 * failed log, logs without a hit — searches them sequentially, maps the hits to elements by a plain scan, and runs select, the two scans and emit through
 * emu_replace.cc in the three lane orders for several patterns and replacement lengths, against the sequential greedy loop below.  Every buffer is exactly as
 * large as the library makes it — the hit and flag arrays end at the last hit, `pre` at pre[n_visible] of the last good log, the op columns at the last op — so
 * a read of hit 64 of a tile of 63, or a store one op too far, is the sanitizer's finding.
 */
#include "emu_replace.cc"

#include <stdio.h>

#include <string>
#include <vector>

static uint32_t g_rng = 4211u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

struct Log {
    uint32_t status;
    std::vector<std::string> elems;
};

struct Op {
    uint8_t action;
    uint32_t index, count;
};

static int run(const std::vector<Log>& logs, uint32_t first_log, uint32_t n_batch, const std::string& pat, uint32_t nrep, const char* what) {
    const uint32_t n = (uint32_t)logs.size(), m = (uint32_t)pat.size();
    /* the view's part: status, prefix, hits — sequentially */
    std::vector<uint32_t> status(n), pre, hu, hs, he;
    std::vector<uint64_t> pre_off(n + 1, 0), hit_off(n + 1, 0);
    /* the expectation */
    std::vector<uint32_t> want_sel, want_status(n), want_c(n, 0), want_r(n, 0);
    std::vector<std::vector<Op>> want_ops(n);
    for (uint32_t l = 0; l < n; ++l) {
        status[l] = want_status[l] = logs[l].status;
        if (logs[l].status == PTX_OK) {
            std::string text;
            std::vector<uint32_t> p;
            for (const std::string& e : logs[l].elems) p.push_back((uint32_t)text.size()), text += e;
            p.push_back((uint32_t)text.size());
            const uint32_t nv = (uint32_t)logs[l].elems.size();
            uint32_t limit = 0, rank = 0;
            uint64_t rows = 0;
            std::vector<Op> desc;
            for (size_t u = 0; u + m <= text.size(); ++u) {
                if (text.compare(u, m, pat) != 0) continue;
                uint32_t s = 0, e = 0;
                for (uint32_t el = 0; el < nv; ++el) { /* the element that holds a unit: pre[el] <= u < pre[el + 1] */
                    if (p[el] <= u && u < p[el + 1]) s = el;
                    if (p[el] <= u + m - 1 && u + m - 1 < p[el + 1]) e = el + 1;
                }
                hu.push_back((uint32_t)u), hs.push_back(s), he.push_back(e);
                uint32_t flag = 0;
                if (u >= limit) { /* the sequential greedy loop */
                    limit = (uint32_t)u + m;
                    ++want_c[l];
                    flag = 1;
                    if (p[s] == u && p[e] == u + m) {
                        flag = 2 + rank++;
                        rows += e - s;
                        desc.push_back(Op{(uint8_t)PTX_IN_DELETE, s, e - s});
                    }
                }
                want_sel.push_back(flag);
            }
            want_r[l] = rank;
            rows += (uint64_t)rank * nrep;
            if (rows > PTX_CHANGE_ROWS_MAX) want_status[l] = PTX_ERR_CAPACITY;
            else
                for (size_t i = desc.size(); i-- > 0;) {
                    want_ops[l].push_back(desc[i]);
                    if (nrep) want_ops[l].push_back(Op{(uint8_t)PTX_IN_INSERT, desc[i].index, nrep});
                }
            pre.insert(pre.end(), p.begin(), p.end());
        }
        pre_off[l + 1] = pre.size();
        hit_off[l + 1] = hu.size();
    }
    const uint32_t nh = (uint32_t)hu.size();
    uint64_t want_changes = 0, want_ni = 0;
    for (uint32_t l = 0; l < n; ++l) want_changes += !want_ops[l].empty(), want_ni += want_ops[l].size();
    EmuReplaceIn in{status.data(), pre_off.data(), pre.data(), hit_off.data(), hu.data(), hs.data(), he.data(), n, m, nrep, first_log, n_batch};
    for (int reverse = 0; reverse < 3; ++reverse) {
        std::vector<uint32_t> sel(nh, 0xA5A5A5A5u), st(n, 0xA5A5A5A5u), nc(n, 0xA5A5A5A5u), nr(n, 0xA5A5A5A5u), nops(n, 0xA5A5A5A5u), makes(n_batch, 0xA5A5A5A5u);
        std::vector<uint64_t> chg(n_batch + 1, ~0ull), olo(n + 1, ~0ull);
        int rc = ptx_emu_replace_select(&in, reverse, sel.data(), st.data(), nc.data(), nr.data(), nops.data(), makes.data(), chg.data(), olo.data());
        if (rc != 0) return printf("%s: select rc %d\n", what, rc), 1;
        for (uint32_t k = 0; k < nh; ++k)
            if (sel[k] != want_sel[k]) return printf("%s order %d hit %u: flag %u, want %u\n", what, reverse, k, sel[k], want_sel[k]), 1;
        for (uint32_t l = 0; l < n; ++l) {
            if (st[l] != want_status[l] || nc[l] != want_c[l] || nr[l] != want_r[l])
                return printf("%s order %d log %u: status %u chosen %u replaced %u, want %u %u %u\n", what, reverse, l, st[l], nc[l], nr[l], want_status[l], want_c[l], want_r[l]), 1;
            if (nops[l] != want_ops[l].size()) return printf("%s order %d log %u: %u ops, want %zu\n", what, reverse, l, nops[l], want_ops[l].size()), 1;
        }
        if (chg[n_batch] != want_changes || olo[n] != want_ni) return printf("%s order %d: %llu Changes, want %llu\n", what, reverse, (unsigned long long)chg[n_batch], (unsigned long long)want_changes), 1;
        for (uint32_t b = 0; b < n_batch; ++b) {
            const bool inside = b >= first_log && b - first_log < n;
            const uint64_t makes_one = inside && !want_ops[b - first_log].empty() ? 1 : 0;
            if (chg[b + 1] - chg[b] != makes_one) return printf("%s order %d batch log %u: chg_off\n", what, reverse, b), 1;
        }
        const uint64_t ni = olo[n];
        std::vector<uint64_t> oo(chg[n_batch] + 1, ~0ull);
        std::vector<uint8_t> ac(ni, 0xA5), mt(ni, 0xA5);
        std::vector<uint32_t> ix(ni, 0xA5A5A5A5u), ct(ni, 0xA5A5A5A5u), pl(ni, 0xA5A5A5A5u);
        rc = ptx_emu_replace_emit(&in, reverse, sel.data(), nr.data(), nops.data(), chg.data(), olo.data(), oo.data(), ac.data(), mt.data(), ix.data(), ct.data(), pl.data());
        if (rc != 0) return printf("%s: emit rc %d\n", what, rc), 1;
        uint64_t c = 0, at = 0;
        for (uint32_t l = 0; l < n; ++l) {
            if (want_ops[l].empty()) continue;
            if (oo[c] != at) return printf("%s order %d Change %llu: op_off %llu, want %llu\n", what, reverse, (unsigned long long)c, (unsigned long long)oo[c], (unsigned long long)at), 1;
            for (const Op& w : want_ops[l]) {
                if (ac[at] != w.action || mt[at] != 0 || ix[at] != w.index || ct[at] != w.count || pl[at] != 0)
                    return printf("%s order %d log %u op %llu: (%u, %u, %u), want (%u, %u, %u)\n", what, reverse, l, (unsigned long long)at, ac[at], ix[at], ct[at], w.action, w.index, w.count), 1;
                ++at;
            }
            ++c;
        }
        if (oo[c] != at || at != ni) return printf("%s order %d: the last op_off\n", what, reverse), 1;
    }
    return 0;
}

static Log chain(uint32_t n) {
    Log g{PTX_OK, {}};
    for (uint32_t i = 0; i < n; ++i) g.elems.push_back("a");
    return g;
}

static Log mix(uint32_t n, const std::vector<std::string>& pick) {
    Log g{PTX_OK, {}};
    for (uint32_t i = 0; i < n; ++i) g.elems.push_back(pick[rnd((uint32_t)pick.size())]);
    return g;
}

int main() {
    const uint32_t S = PTX_REPLACE_TILE;
    int bad = 0;
    std::vector<Log> logs;
    for (uint32_t n : {0u, 1u, 2u, 3u, S - 1, S, S + 1, 2 * S, 2 * S + 1, 4 * S + 3}) logs.push_back(chain(n));
    logs.push_back(Log{PTX_ERR_SEQ_GAP, {}});
    for (uint32_t n : {5u, S, 3 * S + 1}) {
        logs.push_back(mix(n, {"a", "b"}));
        logs.push_back(mix(n, {"a", "", "aa", "ab", "aab", "b"})); /* empty strings, hits that start and end inside elements */
    }
    logs.push_back(mix(40, {"x", "y"})); /* no hit */
    logs.push_back(chain(2 * S));        /* the LAST log is dense: its hits end the hit arrays, its prefix ends `pre` */
    const uint32_t n = (uint32_t)logs.size();
    for (const char* pat : {"a", "aa", "aaa", "ab", "aba", "z"})
        for (uint32_t nrep : {0u, 1u, 3u}) {
            bad |= run(logs, 0, n, pat, nrep, "whole batch");
            bad |= run(logs, 3, n + 9, pat, nrep, "a view behind log 3 of a longer batch");
        }
    /* capacity: 65 533 elements per replaced match are the most a log with ONE whole-element match of one element may take; the dense logs are over it with fewer */
    bad |= run(logs, 0, n, "aa", PTX_CHANGE_ROWS_MAX - 2, "capacity, aa");
    bad |= run({chain(1), chain(2), mix(3, {"x"})}, 0, 3, "a", PTX_CHANGE_ROWS_MAX - 1, "capacity, 65533");
    bad |= run({chain(1), chain(2), mix(3, {"x"})}, 0, 3, "a", PTX_CHANGE_ROWS_MAX, "capacity, 65534");
    bad |= run({}, 2, 5, "a", 1, "the empty view");
    if (bad) return 1;
    printf("replace emulation ok\n");
    return 0;
}
