/*
 * Stand-alone sanitizer program of the document-text emulation — TEST TOOLING ONLY (tests/test_emu_text.py compiles it with g++ -fsanitize=address,undefined and
 * runs it as a child process).  It builds string tables and merge results itself — visible counts around the wave and tile edges, values of 0, 1, 2,
 * threshold - 1 / threshold / threshold + 1 and 5 000 code units, logs that start on odd units, a failed log, a log with a value id beyond the table, ranges that
 * start behind log 0 — runs both passes of text_core.h through emu_text.cc in the three lane orders and compares with the sequential join below.  Every buffer
 * is exactly as large as the host library makes it, so a store or a load one unit too far is the sanitizer's finding.
 */
#include "emu_text.cc"

#include <stdio.h>

#include <algorithm>
#include <vector>

static uint32_t g_rng = 2024u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

struct Table {
    std::vector<uint16_t> units;
    std::vector<uint64_t> off;
    uint32_t n() const { return (uint32_t)off.size() - 1u; }
};
static Table make_table(const std::vector<uint32_t>& lens) {
    Table t;
    t.off.push_back(0);
    for (uint32_t n : lens) {
        for (uint32_t u = 0; u < n; ++u) t.units.push_back((uint16_t)(0x100u * (t.off.size() & 0xFFu) + (u & 0xFFu) + 1u));
        t.off.push_back(t.units.size());
    }
    return t;
}

struct LogIn {
    uint32_t status; /* the merge's */
    std::vector<uint32_t> ids;
    std::vector<uint32_t> span_start;
    uint32_t slack; /* rows of the log beyond its visible elements (a log has at least as many ops as rows) */
};

static int run(const Table& t, const std::vector<LogIn>& in, uint32_t first, uint32_t count, const char* what) {
    const uint32_t L = (uint32_t)in.size();
    std::vector<uint64_t> log_off(L + 1, 0);
    for (uint32_t l = 0; l < L; ++l) log_off[l + 1] = log_off[l] + std::max(in[l].ids.size(), in[l].span_start.size()) + in[l].slack;
    std::vector<ptx_log_result> logs(L);
    std::vector<uint32_t> values(log_off[L], 0xDEADBEEFu); /* rows no element stands in hold an id far beyond any table: reading one would show */
    std::vector<ptx_span> spans(log_off[L], ptx_span{0xDEADBEEFu, 0u});
    memset(logs.data(), 0, L * sizeof(ptx_log_result));
    for (uint32_t l = 0; l < L; ++l) {
        logs[l].status = in[l].status;
        if (in[l].status != PTX_OK) continue;
        logs[l].n_visible = (uint32_t)in[l].ids.size();
        logs[l].n_spans = (uint32_t)in[l].span_start.size();
        for (size_t i = 0; i < in[l].ids.size(); ++i) values[log_off[l] + i] = in[l].ids[i];
        for (size_t k = 0; k < in[l].span_start.size(); ++k) spans[log_off[l] + k] = ptx_span{in[l].span_start[k], (uint32_t)k};
    }
    /* the sequential join */
    std::vector<uint32_t> want_status(count);
    std::vector<std::vector<uint16_t>> want_text(count);
    std::vector<std::vector<uint32_t>> want_unit(count);
    for (uint32_t k = 0; k < count; ++k) {
        const LogIn& g = in[first + k];
        want_status[k] = g.status;
        if (g.status != PTX_OK) continue;
        bool bad = false;
        for (uint32_t id : g.ids) bad |= id >= t.n();
        want_unit[k].assign(g.span_start.size(), 0u);
        if (bad) {
            want_status[k] = PTX_ERR_BAD_OP;
            continue;
        }
        std::vector<uint32_t> at;
        for (uint32_t id : g.ids) {
            at.push_back((uint32_t)want_text[k].size());
            for (uint64_t u = t.off[id]; u < t.off[id + 1]; ++u) want_text[k].push_back(t.units[u]);
        }
        for (size_t s = 0; s < g.span_start.size(); ++s) want_unit[k][s] = at[g.span_start[s]];
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
        const uint64_t* soff = off.data() + count + 1;
        for (uint32_t k = 0; k < count; ++k) {
            if (status[k] != want_status[k]) return printf("%s order %d log %u: status %u, want %u\n", what, reverse, k, status[k], want_status[k]), 1;
            if (off[k + 1] - off[k] != want_text[k].size()) return printf("%s order %d log %u: %llu units, want %zu\n", what, reverse, k, (unsigned long long)(off[k + 1] - off[k]), want_text[k].size()), 1;
            if (!want_text[k].empty() && memcmp(text.data() + off[k], want_text[k].data(), 2 * want_text[k].size()) != 0) return printf("%s order %d log %u: text differs\n", what, reverse, k), 1;
            if (soff[k + 1] - soff[k] != want_unit[k].size()) return printf("%s order %d log %u: span count\n", what, reverse, k), 1;
            for (size_t s = 0; s < want_unit[k].size(); ++s)
                if (unit[soff[k] + s] != want_unit[k][s]) return printf("%s order %d log %u span %zu: unit %u, want %u\n", what, reverse, k, s, unit[soff[k] + s], want_unit[k][s]), 1;
        }
    }
    return 0;
}

/* n elements with ids from `pick`, spans at every `every`-th element (and always at 0) */
static LogIn make_log(uint32_t n, const std::vector<uint32_t>& pick, uint32_t every, uint32_t slack = 1) {
    LogIn g{PTX_OK, {}, {}, slack};
    for (uint32_t i = 0; i < n; ++i) {
        g.ids.push_back(pick[rnd((uint32_t)pick.size())]);
        if (i == 0 || (every && i % every == 0) || (!every && rnd(7) == 0)) g.span_start.push_back(i);
    }
    return g;
}

int main() {
    const uint32_t T = PTX_TEXT_TILE, M = PTX_TEXT_LANE_MAX;
    const uint32_t counts[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1};
    int bad = 0;
    /* every value one unit: the packed stores, logs of odd length so that later logs start on odd units */
    {
        const Table t = make_table(std::vector<uint32_t>(128, 1u));
        std::vector<uint32_t> all;
        for (uint32_t i = 0; i < 128; ++i) all.push_back(i);
        std::vector<LogIn> in;
        for (uint32_t n : counts) in.push_back(make_log(n, all, 0));
        for (uint32_t n : counts) in.push_back(make_log(n | 1u, all, 1, 0)); /* a span per element, no spare rows */
        bad |= run(t, in, 0, (uint32_t)in.size(), "one-unit");
        bad |= run(t, in, 3, (uint32_t)in.size() - 5, "one-unit range");
        bad |= run(t, in, 4, 0, "empty range");
    }
    /* values of every length class; an empty string and spans made only of them; a 5 000-unit value */
    {
        const Table t = make_table({1, 0, 2, M - 1, M, M + 1, 5000, 1, 3, 0});
        std::vector<LogIn> in;
        for (uint32_t n : counts) in.push_back(make_log(n, {0, 1, 2, 3, 4, 5, 7, 8, 9}, 0));
        in.push_back(make_log(T + 3, {1, 9}, 1));    /* tiles of empty strings only */
        in.push_back(make_log(70, {6, 0, 5}, 3));    /* wave copies */
        LogIn edge = make_log(2 * T, {0}, 5);
        edge.ids[0] = 2, edge.ids[T - 1] = 6, edge.ids[T] = 5, edge.ids[2 * T - 1] = 4; /* multi-unit values first, across the tile edge, last */
        in.push_back(edge);
        LogIn failed{PTX_ERR_SEQ_GAP, {}, {}, 9};
        in.push_back(failed);
        LogIn oob = make_log(T + 2, {0, 2}, 4);
        oob.ids[T + 1] = t.n(); /* the first id beyond the table, in the second tile */
        in.push_back(oob);
        in.push_back(make_log(65, {0, 2, 3}, 2));
        bad |= run(t, in, 0, (uint32_t)in.size(), "mixed");
        bad |= run(t, in, 9, (uint32_t)in.size() - 9, "mixed range");
    }
    /* an empty table: every id is beyond it */
    {
        Table t;
        t.off.push_back(0);
        t.units.push_back(0); /* (the library allocates at least one unit) */
        std::vector<LogIn> in = {make_log(0, {0}, 0), make_log(5, {0}, 0)};
        bad |= run(t, in, 0, 2, "empty table");
    }
    if (bad) return 1;
    printf("text emulation ok\n");
    return 0;
}
