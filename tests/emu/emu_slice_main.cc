/*
 * Stand-alone sanitizer program of the slice emulation — TEST TOOLING ONLY (tests/test_emu_slices.py compiles it with g++ -fsanitize=address,undefined and runs it
 * as a child process).  It builds string tables and merge results itself — logs around the tile edges with values of 0, 1, 2 and many units, span rows on every
 * other element, an empty log, a failed log, a log with a value id beyond the table — and slice lists — bounds around the tile and the log's end, 0xFFFFFFFF,
 * empty, reversed, repeated and whole-log slices, logs without slices, runs of empty slices, one-unit slices beyond a block — runs the text passes and then the
 * slice passes through emu_slice.cc in the three lane orders, and compares with the sequential cut below.  Every buffer is exactly as large as the host library
 * makes it, so a gather one element past a prefix, or a store one unit too far, is the sanitizer's finding.
 */
#include "emu_slice.cc"

#include <stdio.h>

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
    std::vector<ptx_span> spans;
    uint32_t slack;
    std::vector<std::pair<uint32_t, uint32_t>> slices;
};

static int run(const Table& t, const std::vector<LogIn>& in, uint32_t first, uint32_t count, const char* what) {
    const uint32_t L = (uint32_t)in.size();
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
        logs[l].n_spans = (uint32_t)in[l].spans.size();
        for (size_t i = 0; i < in[l].ids.size(); ++i) values[log_off[l] + i] = in[l].ids[i];
        for (size_t i = 0; i < in[l].spans.size(); ++i) spans[log_off[l] + i] = in[l].spans[i];
    }
    /* the slice lists of the range, and the sequential cut */
    std::vector<uint64_t> slice_off(count + 1, 0);
    std::vector<uint32_t> ss, se, want_status(count), want_a, want_b;
    std::vector<std::vector<uint16_t>> want_text;
    std::vector<std::vector<ptx_span>> want_rows;
    std::vector<std::vector<uint32_t>> want_unit;
    for (uint32_t k = 0; k < count; ++k) {
        const LogIn& g = in[first + k];
        uint32_t st = g.status;
        if (st == PTX_OK)
            for (uint32_t id : g.ids)
                if (id >= t.n()) st = PTX_ERR_BAD_OP;
        want_status[k] = st;
        const uint32_t nv = st == PTX_OK ? (uint32_t)g.ids.size() : 0u;
        for (auto& sl : g.slices) {
            ss.push_back(sl.first);
            se.push_back(sl.second);
            uint32_t a = sl.first < nv ? sl.first : nv, b = sl.second < nv ? sl.second : nv;
            if (a >= b) b = a;
            want_a.push_back(a);
            want_b.push_back(b);
            std::vector<uint16_t> txt;
            std::vector<ptx_span> rows;
            std::vector<uint32_t> unit;
            for (uint32_t e = a; e < b; ++e) {
                for (size_t q = 0; q < g.spans.size(); ++q) { /* the row that holds element e opens a row of the slice at its first element inside it */
                    const uint32_t s0 = g.spans[q].start, s1 = q + 1 < g.spans.size() ? g.spans[q + 1].start : nv;
                    if (s0 <= e && e < s1 && (e == a || e == s0)) {
                        rows.push_back(ptx_span{e, g.spans[q].attr});
                        unit.push_back((uint32_t)txt.size());
                    }
                }
                for (uint64_t u = t.off[g.ids[e]]; u < t.off[g.ids[e] + 1]; ++u) txt.push_back(t.units[u]);
            }
            want_text.push_back(txt);
            want_rows.push_back(rows);
            want_unit.push_back(unit);
        }
        slice_off[k + 1] = ss.size();
    }
    const uint32_t ns = (uint32_t)ss.size();
    for (int reverse = 0; reverse < 3; ++reverse) {
        std::vector<uint32_t> status(count ? count : 1, 0xA5A5A5A5u);
        std::vector<uint64_t> off(2 * ((size_t)count + 1), 0xA5A5A5A5A5A5A5A5ull);
        int rc = ptx_emu_text_lengths(log_off.data(), L, logs.data(), values.data(), spans.data(), t.units.data(), t.off.data(), t.n(), first, count, reverse, status.data(), off.data());
        if (rc != 0) return printf("%s: lengths rc %d\n", what, rc), 1;
        std::vector<uint16_t> text(off[count], 0xA5A5u);
        std::vector<uint32_t> unit(off[2 * (size_t)count + 1], 0xA5A5A5A5u);
        rc = ptx_emu_text_assemble(log_off.data(), logs.data(), values.data(), spans.data(), t.units.data(), t.off.data(), t.n(), first, count, reverse, status.data(), off.data(),
                                   text.data(), unit.data());
        if (rc != 0) return printf("%s: assemble rc %d\n", what, rc), 1;
        std::vector<uint32_t> ea(ns, 0xA5A5A5A5u), eb(ns, 0xA5A5A5A5u);
        std::vector<uint64_t> out_off(2 * ((size_t)ns + 1), 0xA5A5A5A5A5A5A5A5ull);
        EmuSlices* h = nullptr;
        rc = ptx_emu_slices_bounds(log_off.data(), L, logs.data(), values.data(), spans.data(), t.off.data(), t.n(), first, count, status.data(), off.data(), text.data(), slice_off.data(),
                                   ss.data(), se.data(), reverse, ea.data(), eb.data(), out_off.data(), &h);
        if (rc != 0) return printf("%s: bounds rc %d\n", what, rc), 1;
        const uint64_t* unit_off = out_off.data();
        const uint64_t* sspan_off = out_off.data() + ns + 1;
        std::vector<uint16_t> ot(unit_off[ns], 0xA5A5u);
        std::vector<ptx_span> os(sspan_off[ns], ptx_span{0xA5A5A5A5u, 0xA5A5A5A5u});
        std::vector<uint32_t> ou(sspan_off[ns], 0xA5A5A5A5u);
        rc = ptx_emu_slices_emit(h, reverse, ot.data(), os.data(), ou.data());
        ptx_emu_slices_close(h);
        if (rc != 0) return printf("%s: emit rc %d\n", what, rc), 1;
        for (uint32_t k = 0; k < count; ++k)
            if (status[k] != want_status[k]) return printf("%s order %d log %u: status %u, want %u\n", what, reverse, k, status[k], want_status[k]), 1;
        for (uint32_t k = 0; k < ns; ++k) {
            if (ea[k] != want_a[k] || eb[k] != want_b[k]) return printf("%s order %d slice %u: [%u, %u), want [%u, %u)\n", what, reverse, k, ea[k], eb[k], want_a[k], want_b[k]), 1;
            if (unit_off[k + 1] - unit_off[k] != want_text[k].size()) return printf("%s order %d slice %u: %llu units, want %zu\n", what, reverse, k, (unsigned long long)(unit_off[k + 1] - unit_off[k]), want_text[k].size()), 1;
            for (size_t u = 0; u < want_text[k].size(); ++u)
                if (ot[unit_off[k] + u] != want_text[k][u]) return printf("%s order %d slice %u unit %zu: %04x, want %04x\n", what, reverse, k, u, ot[unit_off[k] + u], want_text[k][u]), 1;
            if (sspan_off[k + 1] - sspan_off[k] != want_rows[k].size()) return printf("%s order %d slice %u: %llu rows, want %zu\n", what, reverse, k, (unsigned long long)(sspan_off[k + 1] - sspan_off[k]), want_rows[k].size()), 1;
            for (size_t q = 0; q < want_rows[k].size(); ++q) {
                const uint64_t at = sspan_off[k] + q;
                if (os[at].start != want_rows[k][q].start || os[at].attr != want_rows[k][q].attr || ou[at] != want_unit[k][q])
                    return printf("%s order %d slice %u row %zu: (%u, %u, %u), want (%u, %u, %u)\n", what, reverse, k, q, os[at].start, os[at].attr, ou[at], want_rows[k][q].start, want_rows[k][q].attr, want_unit[k][q]), 1;
            }
        }
    }
    return 0;
}

static LogIn make_log(uint32_t n, const std::vector<uint32_t>& pick, uint32_t span_every, uint32_t slack = 1) {
    LogIn g{PTX_OK, {}, {}, slack, {}};
    for (uint32_t i = 0; i < n; ++i) g.ids.push_back(pick[rnd((uint32_t)pick.size())]);
    for (uint32_t i = 0; i < n; i += span_every) g.spans.push_back(ptx_span{i, 1u + (i & 0xFFu)});
    return g;
}

static void edge_slices(LogIn& g) {
    const uint32_t T = PTX_TEXT_TILE, n = (uint32_t)g.ids.size();
    const uint32_t pts[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T, n ? n - 1 : 0, n, n + 1, 0xFFFFFFFFu};
    for (uint32_t a : pts)
        for (uint32_t b : pts) g.slices.push_back({a, b}); /* empty and reversed ones included */
    for (int i = 0; i < 3; ++i) g.slices.push_back({2, 9});  /* the same slice three times */
    for (int i = 0; i < 20; ++i) {
        const uint32_t a = rnd(n + 2), b = rnd(n + 2);
        g.slices.push_back({a, b});
    }
}

int main() {
    const uint32_t T = PTX_TEXT_TILE, B = PTX_SLICE_BLOCK;
    int bad = 0;
    /* 0 "a", 1 "b", 2 "", 3 "ab", 4 a value of 5 000 units, 5 "bab" */
    Table t;
    t.off.push_back(0);
    t.add({0x61});
    t.add({0x62});
    t.add({});
    t.add({0x61, 0x62});
    {
        std::vector<uint16_t> big;
        for (uint32_t i = 0; i < 5000; ++i) big.push_back((uint16_t)(0x4E00 + rnd(500)));
        t.add(big);
    }
    t.add({0x62, 0x61, 0x62});
    const uint32_t counts[] = {0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1};
    std::vector<LogIn> in;
    for (uint32_t n : counts) {
        in.push_back(make_log(n, {0, 1}, 1, n & 1u)); /* one unit per element, a row per element */
        edge_slices(in.back());
        in.push_back(make_log(n, {0, 1, 2, 3, 5}, 3)); /* empty strings, two- and three-unit values: every parity at heads and tails */
        edge_slices(in.back());
        in.push_back(make_log(n, {0, 1}, 7)); /* a log without slices between logs with them */
    }
    {
        LogIn g = make_log(T + 5, {2}, 2); /* empty strings only, then "a", "", "b" */
        g.ids[T + 1] = 0, g.ids[T + 2] = 2, g.ids[T + 3] = 1;
        edge_slices(g);
        in.push_back(g);
    }
    {
        LogIn g = make_log(2 * T, {0, 1}, 5); /* the long value first, at the tile edge, last; as slices of their own: the output crosses many blocks */
        g.ids[0] = 4, g.ids[T - 1] = 4, g.ids[T] = 3, g.ids[2 * T - 1] = 4;
        g.slices = {{0, 1}, {T - 1, T + 1}, {2 * T - 1, 2 * T}, {0, 0xFFFFFFFFu}, {1, 2}};
        in.push_back(g);
    }
    in.push_back(LogIn{PTX_ERR_SEQ_GAP, {}, {}, 9, {{0, 5}, {3, 3}}});
    {
        LogIn g = make_log(T + 2, {0, 1}, 4);
        g.ids[T + 1] = t.n(); /* the first id beyond the table */
        g.slices = {{0, 5}, {T, T + 2}};
        in.push_back(g);
    }
    {
        LogIn g = make_log(B + 40, {0, 1}, 11); /* B + 1 one-unit slices in a row, 65 empty slices between two non-empty ones, output ends at B - 1, B, B + 1 */
        for (uint32_t i = 0; i <= B; ++i) g.slices.push_back({i, i + 1});
        g.slices.push_back({0, B - 2});
        for (int i = 0; i < 65; ++i) g.slices.push_back({7, 7});
        g.slices.push_back({3, 4});
        in.push_back(g);
    }
    const uint32_t N = (uint32_t)in.size();
    bad |= run(t, in, 0, N, "whole batch");
    bad |= run(t, in, 5, N - 7, "a range behind log 0");
    bad |= run(t, in, 2, 1, "one log without slices");
    bad |= run(t, in, 4, 0, "empty range");
    if (bad) return 1;
    printf("slice emulation ok\n");
    return 0;
}
