/*
 * Stand-alone sanitizer program of the find emulation — TEST TOOLING ONLY (tests/test_emu_find.py compiles it with g++ -fsanitize=address,undefined and runs it
 * as a child process).  It builds string tables and merge results itself — texts around the step edges, logs of odd lengths back to back, empty logs, a failed
 * log, a log with a value id beyond the table, values of 0, 1, 2 and many units around the tile edges, dense texts — runs the text passes and then count, scan
 * and emit through emu_find.cc in the three lane orders, for patterns of 1 .. PTX_FIND_PATTERN_MAX units and several caps, and compares with the
 * sequential search below.  Every buffer is exactly as large as the host library makes it (the text buffer ends with the last log's last unit), so a halo that
 * reaches past a log's end into nothing, or a store one word too far, is the sanitizer's finding.
 */
#include "emu_find.cc"

#include <stdio.h>

#include <algorithm>
#include <vector>

static uint32_t g_rng = 4711u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

struct Table {
    std::vector<uint16_t> units;
    std::vector<uint64_t> off;
    uint32_t n() const { return (uint32_t)off.size() - 1u; }
    void add(const std::vector<uint16_t>& s) {
        units.insert(units.end(), s.begin(), s.end());
        off.push_back(units.size());
    }
};

struct LogIn {
    uint32_t status; /* the merge's */
    std::vector<uint32_t> ids;
    uint32_t slack;
};

static uint16_t foldu(uint16_t u, bool nocase) { return nocase && u >= 0x41 && u <= 0x5A ? (uint16_t)(u + 0x20) : u; }

static int run(const Table& t, const std::vector<LogIn>& in, uint32_t first, uint32_t count, const std::vector<uint16_t>& pat, uint32_t flags, uint32_t cap, const char* what) {
    const uint32_t L = (uint32_t)in.size(), m = (uint32_t)pat.size();
    std::vector<uint64_t> log_off(L + 1, 0);
    for (uint32_t l = 0; l < L; ++l) log_off[l + 1] = log_off[l] + in[l].ids.size() + in[l].slack;
    std::vector<ptx_log_result> logs(L);
    std::vector<uint32_t> values(log_off[L], 0xDEADBEEFu); /* rows no element stands in hold an id far beyond any table: reading one would show */
    std::vector<ptx_span> spans(log_off[L], ptx_span{0xDEADBEEFu, 0u});
    memset(logs.data(), 0, L * sizeof(ptx_log_result));
    for (uint32_t l = 0; l < L; ++l) {
        logs[l].status = in[l].status;
        if (in[l].status != PTX_OK) continue;
        logs[l].n_visible = (uint32_t)in[l].ids.size();
        for (size_t i = 0; i < in[l].ids.size(); ++i) values[log_off[l] + i] = in[l].ids[i];
    }
    /* the sequential search */
    std::vector<uint32_t> want_status(count), want_n(count);
    std::vector<std::vector<uint32_t>> want_u(count), want_s(count), want_e(count);
    for (uint32_t k = 0; k < count; ++k) {
        const LogIn& g = in[first + k];
        want_status[k] = g.status;
        if (g.status != PTX_OK) continue;
        bool bad = false;
        for (uint32_t id : g.ids) bad |= id >= t.n();
        if (bad) {
            want_status[k] = PTX_ERR_BAD_OP;
            continue;
        }
        std::vector<uint16_t> text;
        std::vector<uint32_t> holder; /* per unit: its element */
        for (size_t e = 0; e < g.ids.size(); ++e)
            for (uint64_t u = t.off[g.ids[e]]; u < t.off[g.ids[e] + 1]; ++u) {
                text.push_back(t.units[u]);
                holder.push_back((uint32_t)e);
            }
        for (size_t p = 0; p + m <= text.size(); ++p) {
            bool eq = true;
            for (uint32_t i = 0; i < m && eq; ++i) eq = foldu(text[p + i], flags & 1u) == foldu(pat[i], flags & 1u);
            if (!eq) continue;
            if (want_n[k]++ < cap) {
                want_u[k].push_back((uint32_t)p);
                want_s[k].push_back(holder[p]);
                want_e[k].push_back(holder[p + m - 1] + 1u);
            }
        }
    }
    for (int reverse = 0; reverse < 3; ++reverse) {
        std::vector<uint32_t> status(count, 0xA5A5A5A5u);
        std::vector<uint64_t> off(2 * ((size_t)count + 1), 0xA5A5A5A5A5A5A5A5ull);
        int rc = ptx_emu_text_lengths(log_off.data(), L, logs.data(), values.data(), spans.data(), t.units.data(), t.off.data(), t.n(), first, count, reverse, status.data(), off.data());
        if (rc != 0) return printf("%s: lengths rc %d\n", what, rc), 1;
        std::vector<uint16_t> text(off[count], 0xA5A5u);
        std::vector<uint32_t> unit(off[2 * (size_t)count + 1], 0xA5A5A5A5u);
        rc = ptx_emu_text_assemble(log_off.data(), logs.data(), values.data(), spans.data(), t.units.data(), t.off.data(), t.n(), first, count, reverse, status.data(), off.data(),
                                   text.data(), unit.data());
        if (rc != 0) return printf("%s: assemble rc %d\n", what, rc), 1;
        std::vector<uint32_t> n_matches(count, 0xA5A5A5A5u);
        std::vector<uint64_t> hit_off((size_t)count + 1, 0xA5A5A5A5A5A5A5A5ull);
        rc = ptx_emu_find_count(status.data(), off.data(), text.data(), count, pat.data(), m, flags, cap, reverse, n_matches.data(), hit_off.data());
        if (rc != 0) return printf("%s: count rc %d\n", what, rc), 1;
        std::vector<uint32_t> hu(hit_off[count], 0xA5A5A5A5u), hs(hit_off[count], 0xA5A5A5A5u), he(hit_off[count], 0xA5A5A5A5u);
        rc = ptx_emu_find_emit(log_off.data(), logs.data(), values.data(), t.off.data(), t.n(), first, count, status.data(), off.data(), text.data(), pat.data(), m, flags, cap, reverse,
                               hit_off.data(), hu.data(), hs.data(), he.data());
        if (rc != 0) return printf("%s: emit rc %d\n", what, rc), 1;
        for (uint32_t k = 0; k < count; ++k) {
            if (status[k] != want_status[k]) return printf("%s order %d log %u: status %u, want %u\n", what, reverse, k, status[k], want_status[k]), 1;
            if (n_matches[k] != want_n[k]) return printf("%s order %d log %u: %u matches, want %u\n", what, reverse, k, n_matches[k], want_n[k]), 1;
            if (hit_off[k + 1] - hit_off[k] != want_u[k].size()) return printf("%s order %d log %u: %llu listed, want %zu\n", what, reverse, k, (unsigned long long)(hit_off[k + 1] - hit_off[k]), want_u[k].size()), 1;
            for (size_t j = 0; j < want_u[k].size(); ++j) {
                const uint64_t at = hit_off[k] + j;
                if (hu[at] != want_u[k][j] || hs[at] != want_s[k][j] || he[at] != want_e[k][j])
                    return printf("%s order %d log %u hit %zu: (%u, %u, %u), want (%u, %u, %u)\n", what, reverse, k, j, hu[at], hs[at], he[at], want_u[k][j], want_s[k][j], want_e[k][j]), 1;
            }
        }
    }
    return 0;
}

static LogIn make_log(uint32_t n, const std::vector<uint32_t>& pick, uint32_t slack = 1) {
    LogIn g{PTX_OK, {}, slack};
    for (uint32_t i = 0; i < n; ++i) g.ids.push_back(pick[rnd((uint32_t)pick.size())]);
    return g;
}

int main() {
    const uint32_t S = PTX_FIND_STEP, T = PTX_TEXT_TILE, P = PTX_FIND_PATTERN_MAX;
    int bad = 0;
    /* a table over a two-letter alphabet, so that every pattern hits often: 0 "a", 1 "b", 2 "", 3 "ab", 4 "A", 5 a value of 700 units of a's and b's, 6 "ba" */
    Table t;
    t.off.push_back(0);
    t.add({0x61});
    t.add({0x62});
    t.add({});
    t.add({0x61, 0x62});
    t.add({0x41});
    {
        std::vector<uint16_t> big;
        for (uint32_t i = 0; i < 700; ++i) big.push_back((uint16_t)(0x61 + rnd(2)));
        t.add(big);
    }
    t.add({0x62, 0x61});
    const uint32_t counts[] = {0, 1, 2, 3, 63, 65, S - 1, S, S + 1, S + 2, 2 * S + 1, T - 1, T + 1, 2 * T + 3};
    std::vector<LogIn> in;
    for (uint32_t n : counts) in.push_back(make_log(n, {0, 1}, n & 1u));          /* one unit per element */
    for (uint32_t n : counts) in.push_back(make_log(n, {0, 0, 0, 0, 0, 0, 1}, 0)); /* dense */
    for (uint32_t n : counts) in.push_back(make_log(n, {0, 1, 2, 3, 4, 6}));      /* empty strings, two-unit values, a capital */
    in.push_back(make_log(T + 3, {2}));                                           /* tiles of empty strings only: no text */
    {
        LogIn g = make_log(T + 5, {2});
        g.ids[T + 1] = 0, g.ids[T + 2] = 2, g.ids[T + 3] = 1; /* a tile of empty strings, then "a", "", "b" */
        in.push_back(g);
    }
    {
        LogIn g = make_log(2 * T, {0, 1});
        g.ids[0] = 5, g.ids[T - 1] = 5, g.ids[T] = 3, g.ids[2 * T - 1] = 5; /* long values first, at the tile edge, last */
        in.push_back(g);
    }
    in.push_back(LogIn{PTX_ERR_SEQ_GAP, {}, 9});
    {
        LogIn g = make_log(T + 2, {0, 1});
        g.ids[T + 1] = t.n(); /* the first id beyond the table */
        in.push_back(g);
    }
    in.push_back(make_log(65, {0, 1, 3}));
    const uint32_t N = (uint32_t)in.size();
    const uint32_t lens[] = {1, 2, 3, 5, 64, 65, P - 1, P};
    for (uint32_t m : lens) {
        /* a pattern that occurs: a stretch of the long value; and one of a's only */
        std::vector<uint16_t> from_text(t.units.begin() + t.off[5] + 100, t.units.begin() + t.off[5] + 100 + m), as(m, 0x61);
        char what[64];
        snprintf(what, sizeof(what), "m=%u text", m);
        bad |= run(t, in, 0, N, from_text, 0, 0xFFFFFFFFu, what);
        snprintf(what, sizeof(what), "m=%u a's", m);
        bad |= run(t, in, 0, N, as, 0, 0xFFFFFFFFu, what);
        snprintf(what, sizeof(what), "m=%u a's nocase range", m);
        bad |= run(t, in, 5, N - 7, as, 1, 0xFFFFFFFFu, what);
    }
    const uint32_t caps[] = {0, 1, 63, 64, 65, 2 * S};
    for (uint32_t cap : caps) {
        char what[64];
        snprintf(what, sizeof(what), "cap %u", cap);
        bad |= run(t, in, 0, N, {0x61}, 0, cap, what);
        bad |= run(t, in, 3, N - 3, {0x41, 0x42}, 1, cap, what); /* "AB" against a's and b's: folded on both sides */
    }
    bad |= run(t, in, 0, N, {0x41}, 0, 0xFFFFFFFFu, "capital, exact");
    bad |= run(t, in, 4, 0, {0x61}, 0, 7, "empty range");
    if (bad) return 1;
    printf("find emulation ok\n");
    return 0;
}
