/*
 * Stand-alone sanitizer program of the view emulation — TEST TOOLING ONLY (tests/test_emu_view.py compiles it with g++ -fsanitize=address,undefined and runs it as
 * a child process).  It builds string tables and merge results itself — logs of 0, 1, T - 1, T, T + 1 and 2T + 1 elements with values of 0, 1, 2, 3 and many
 * units, span rows on every third element, a failed log, a log with a value id beyond the table, a log of 2S + 1 equal units — makes a view of a range through
 * emu_view.cc, then runs count, positions, locate, windows, bounds, copy and span emit in the three lane orders for several patterns, caps and windows, and
 * compares with the sequential search and cut below.  Every buffer is exactly as large as the library makes it — the view's `pre` ends at pre[n_visible] of the
 * last good log, the per-hit arrays at the last listed hit — so a locate search that reads one word past a prefix, or a store one hit too far, is the
 * sanitizer's finding.  The arrays a view was made from (log_off, value ids, the string table) are freed before the first query.
 */
#include "emu_view.cc"

#include <stdio.h>

#include <vector>

static uint32_t g_rng = 1789u;
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
};

struct Ask {
    std::vector<uint16_t> pat;
    uint32_t flags, cap, before, after;
};

static uint16_t fold(uint16_t u, bool nocase) { return nocase && u >= 0x41 && u <= 0x5A ? (uint16_t)(u + 0x20) : u; }

static int run(const Table& t, const std::vector<LogIn>& in, uint32_t first, uint32_t count, const std::vector<Ask>& asks, const char* what) {
    const uint32_t L = (uint32_t)in.size();
    std::vector<ptx_log_result> logs(L);
    std::vector<ptx_span> spans;
    memset(logs.data(), 0, L * sizeof(ptx_log_result));
    for (int reverse = 0; reverse < 3; ++reverse) {
        EmuView* v = nullptr;
        {
            /* what the view is made from lives in this block only */
            std::vector<uint64_t> log_off(L + 1, 0);
            for (uint32_t l = 0; l < L; ++l) log_off[l + 1] = log_off[l] + in[l].ids.size() + in[l].slack;
            std::vector<uint32_t> values(log_off[L], 0xDEADBEEFu);
            spans.assign(log_off[L], ptx_span{0xDEADBEEFu, 0u});
            for (uint32_t l = 0; l < L; ++l) {
                logs[l].status = in[l].status;
                if (in[l].status != PTX_OK) continue;
                logs[l].n_visible = (uint32_t)in[l].ids.size();
                logs[l].n_spans = (uint32_t)in[l].spans.size();
                for (size_t i = 0; i < in[l].ids.size(); ++i) values[log_off[l] + i] = in[l].ids[i];
                for (size_t i = 0; i < in[l].spans.size(); ++i) spans[log_off[l] + i] = in[l].spans[i];
            }
            Table copy = t;
            if (copy.units.empty()) copy.units.push_back(0);
            const int rc = ptx_emu_view_create(log_off.data(), L, logs.data(), values.data(), spans.data(), copy.units.data(), copy.off.data(), copy.n(), first, count, reverse, &v);
            if (rc != 0) return printf("%s: create rc %d\n", what, rc), 1;
        }
        /* the sequential answer: status, text and element prefix of every log of the range */
        std::vector<uint32_t> want_status(count);
        std::vector<std::vector<uint16_t>> text(count);
        std::vector<std::vector<uint32_t>> pre(count);
        uint64_t words = 0;
        for (uint32_t k = 0; k < count; ++k) {
            const LogIn& g = in[first + k];
            uint32_t st = g.status;
            if (st == PTX_OK)
                for (uint32_t id : g.ids)
                    if (id >= t.n()) st = PTX_ERR_BAD_OP;
            want_status[k] = st;
            if (st != PTX_OK) continue;
            for (uint32_t id : g.ids) {
                pre[k].push_back((uint32_t)text[k].size());
                for (uint64_t u = t.off[id]; u < t.off[id + 1]; ++u) text[k].push_back(t.units[u]);
            }
            pre[k].push_back((uint32_t)text[k].size());
            words += pre[k].size();
        }
        if (v->n_pre != words) return printf("%s order %d: %llu prefix words, want %llu\n", what, reverse, (unsigned long long)v->n_pre, (unsigned long long)words), 1;
        for (uint32_t k = 0; k < count; ++k) {
            if (v->status[k] != want_status[k]) return printf("%s order %d log %u: status %u, want %u\n", what, reverse, k, v->status[k], want_status[k]), 1;
            for (size_t e = 0; e < pre[k].size(); ++e)
                if (v->pre[v->pre_off[k] + e] != pre[k][e]) return printf("%s order %d log %u: pre[%zu] = %u, want %u\n", what, reverse, k, e, v->pre[v->pre_off[k] + e], pre[k][e]), 1;
        }
        for (size_t qi = 0; qi < asks.size(); ++qi) {
            const Ask& q = asks[qi];
            const uint32_t m = (uint32_t)q.pat.size();
            const bool nocase = (q.flags & PTX_FIND_ASCII_NOCASE) != 0;
            /* sequential search, element mapping, window and cut */
            std::vector<uint32_t> want_n(count, 0), wu, ws, we, wa, wb, wmu, wlog;
            std::vector<uint64_t> want_off(count + 1, 0);
            for (uint32_t k = 0; k < count; ++k) {
                const std::vector<uint16_t>& x = text[k];
                uint32_t listed = 0;
                for (size_t p = 0; p + m <= x.size(); ++p) {
                    bool hit = true;
                    for (uint32_t i = 0; i < m && hit; ++i) hit = fold(x[p + i], nocase) == fold(q.pat[i], nocase);
                    if (!hit) continue;
                    ++want_n[k];
                    if (listed == q.cap) continue;
                    ++listed;
                    const uint32_t nv = (uint32_t)pre[k].size() - 1u;
                    uint32_t s = 0, e = 0;
                    for (uint32_t el = 0; el < nv; ++el) { /* the element that holds a unit: pre[el] <= u < pre[el + 1] */
                        if (pre[k][el] <= p && p < pre[k][el + 1]) s = el;
                        if (pre[k][el] <= p + m - 1 && p + m - 1 < pre[k][el + 1]) e = el + 1;
                    }
                    const uint64_t lo = s > q.before ? s - q.before : 0, hi = (uint64_t)e + q.after;
                    const uint32_t a = (uint32_t)(lo < nv ? lo : nv), b = (uint32_t)(hi < nv ? hi : nv);
                    wu.push_back((uint32_t)p), ws.push_back(s), we.push_back(e), wa.push_back(a), wb.push_back(b), wmu.push_back((uint32_t)p - pre[k][a]), wlog.push_back(k);
                }
                want_off[k + 1] = wu.size();
            }
            const uint32_t nh = (uint32_t)wu.size();
            std::vector<uint32_t> n_matches(count ? count : 1, 0xA5A5A5A5u);
            std::vector<uint64_t> hit_off(count + 1, 0xA5A5A5A5A5A5A5A5ull);
            int rc = ptx_emu_view_count(v, q.pat.data(), m, q.flags, q.cap, reverse, n_matches.data(), hit_off.data());
            if (rc != 0) return printf("%s ask %zu: count rc %d\n", what, qi, rc), 1;
            for (uint32_t k = 0; k < count; ++k)
                if (n_matches[k] != want_n[k] || hit_off[k + 1] != want_off[k + 1]) return printf("%s order %d ask %zu log %u: %u matches, want %u\n", what, reverse, qi, k, n_matches[k], want_n[k]), 1;
            if (hit_off[0] != 0) return printf("%s: hit_off[0]\n", what), 1;
            std::vector<uint32_t> hu(nh, 0xA5A5A5A5u), hs(nh, 0xA5A5A5A5u), he(nh, 0xA5A5A5A5u), w0(nh, 0xA5A5A5A5u), w1(nh, 0xA5A5A5A5u), mu(nh, 0xA5A5A5A5u);
            rc = ptx_emu_view_hits(v, q.pat.data(), m, q.flags, q.cap, reverse, hit_off.data(), hu.data(), hs.data(), he.data(), q.before, q.after, w0.data(), w1.data(), mu.data());
            if (rc != 0) return printf("%s ask %zu: hits rc %d\n", what, qi, rc), 1;
            std::vector<uint32_t> ea(nh, 0xA5A5A5A5u), eb(nh, 0xA5A5A5A5u);
            std::vector<uint64_t> out_off(2 * ((size_t)nh + 1), 0xA5A5A5A5A5A5A5A5ull);
            EmuViewCut* h = nullptr;
            rc = ptx_emu_view_bounds(v, hit_off.data(), w0.data(), w1.data(), 0, reverse, ea.data(), eb.data(), out_off.data(), &h);
            if (rc != 0) return printf("%s ask %zu: bounds rc %d\n", what, qi, rc), 1;
            const uint64_t* unit_off = out_off.data();
            const uint64_t* sspan_off = out_off.data() + nh + 1;
            std::vector<uint16_t> ot(unit_off[nh], 0xA5A5u);
            std::vector<ptx_span> os(sspan_off[nh], ptx_span{0xA5A5A5A5u, 0xA5A5A5A5u});
            std::vector<uint32_t> ou(sspan_off[nh], 0xA5A5A5A5u);
            rc = ptx_emu_view_emit(h, reverse, ot.data(), os.data(), ou.data());
            ptx_emu_view_cut_close(h);
            if (rc != 0) return printf("%s ask %zu: emit rc %d\n", what, qi, rc), 1;
            for (uint32_t k = 0; k < nh; ++k) {
                if (hu[k] != wu[k] || hs[k] != ws[k] || he[k] != we[k])
                    return printf("%s order %d ask %zu hit %u: (%u, %u, %u), want (%u, %u, %u)\n", what, reverse, qi, k, hu[k], hs[k], he[k], wu[k], ws[k], we[k]), 1;
                if (ea[k] != wa[k] || eb[k] != wb[k] || mu[k] != wmu[k])
                    return printf("%s order %d ask %zu snippet %u: [%u, %u) at %u, want [%u, %u) at %u\n", what, reverse, qi, k, ea[k], eb[k], mu[k], wa[k], wb[k], wmu[k]), 1;
                const std::vector<uint16_t>& x = text[wlog[k]];
                const std::vector<uint32_t>& p = pre[wlog[k]];
                const uint32_t len = p[wb[k]] - p[wa[k]];
                if (unit_off[k + 1] - unit_off[k] != len) return printf("%s order %d ask %zu snippet %u: %llu units, want %u\n", what, reverse, qi, k, (unsigned long long)(unit_off[k + 1] - unit_off[k]), len), 1;
                for (uint32_t u = 0; u < len; ++u)
                    if (ot[unit_off[k] + u] != x[p[wa[k]] + u]) return printf("%s order %d ask %zu snippet %u unit %u\n", what, reverse, qi, k, u), 1;
                for (uint32_t i = 0; i < m; ++i) /* the pinned identity */
                    if (fold(ot[unit_off[k] + mu[k] + i], nocase) != fold(q.pat[i], nocase)) return printf("%s order %d ask %zu snippet %u: the pattern is not at match_unit\n", what, reverse, qi, k), 1;
                /* the rows: the row that holds element e opens a row of the snippet at its first element inside it */
                const LogIn& g = in[first + wlog[k]];
                const uint32_t nv = (uint32_t)p.size() - 1u;
                uint64_t at = sspan_off[k];
                for (uint32_t e = wa[k]; e < wb[k]; ++e)
                    for (size_t r = 0; r < g.spans.size(); ++r) {
                        const uint32_t s0 = g.spans[r].start, s1 = r + 1 < g.spans.size() ? g.spans[r + 1].start : nv;
                        if (s0 <= e && e < s1 && (e == wa[k] || e == s0)) {
                            if (at >= sspan_off[k + 1] || os[at].start != e || os[at].attr != g.spans[r].attr || ou[at] != p[e] - p[wa[k]])
                                return printf("%s order %d ask %zu snippet %u: row at element %u\n", what, reverse, qi, k, e), 1;
                            ++at;
                        }
                    }
                if (at != sspan_off[k + 1]) return printf("%s order %d ask %zu snippet %u: too many rows\n", what, reverse, qi, k), 1;
            }
        }
        ptx_emu_view_close(v);
    }
    return 0;
}

static LogIn make_log(uint32_t n, const std::vector<uint32_t>& pick, uint32_t span_every, uint32_t slack = 1) {
    LogIn g{PTX_OK, {}, {}, slack};
    for (uint32_t i = 0; i < n; ++i) g.ids.push_back(pick[rnd((uint32_t)pick.size())]);
    for (uint32_t i = 0; i < n; i += span_every) g.spans.push_back(ptx_span{i, 1u + (i & 0xFFu)});
    return g;
}

int main() {
    const uint32_t T = PTX_TEXT_TILE, S = PTX_FIND_STEP, ALL = 0xFFFFFFFFu;
    int bad = 0;
    /* 0 "a", 1 "b", 2 "", 3 "ab", 4 a value of 700 units, 5 "bab", 6 "A" */
    Table t;
    t.off.push_back(0);
    t.add({0x61});
    t.add({0x62});
    t.add({});
    t.add({0x61, 0x62});
    {
        std::vector<uint16_t> big;
        for (uint32_t i = 0; i < 700; ++i) big.push_back((uint16_t)(0x4E00 + rnd(3)));
        t.add(big);
    }
    t.add({0x62, 0x61, 0x62});
    t.add({0x41});
    const uint32_t counts[] = {0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1};
    std::vector<LogIn> in;
    for (uint32_t n : counts) {
        in.push_back(make_log(n, {0, 1}, 1, n & 1u));        /* one unit per element, a row per element */
        in.push_back(make_log(n, {0, 1, 2, 3, 5, 6}, 3));    /* empty strings, two- and three-unit values */
    }
    {
        LogIn g = make_log(T + 5, {2}, 2); /* empty strings only, then "a", "", "b": the hit "ab" lies across an empty string, behind a tile of them */
        g.ids[T + 1] = 0, g.ids[T + 2] = 2, g.ids[T + 3] = 1;
        in.push_back(g);
    }
    {
        LogIn g = make_log(2 * T, {0, 1}, 5); /* the long value first, at the tile edge, last */
        g.ids[0] = 4, g.ids[T - 1] = 4, g.ids[T] = 3, g.ids[2 * T - 1] = 4;
        in.push_back(g);
    }
    in.push_back(LogIn{PTX_ERR_SEQ_GAP, {}, {}, 9});
    {
        LogIn g = make_log(T + 2, {0, 1}, 4);
        g.ids[T + 1] = t.n(); /* the first id beyond the table */
        in.push_back(g);
    }
    in.push_back(make_log(2 * S + 1, {0}, 7)); /* 2S + 1 x "a": every position hits; the LAST log, so its prefix ends the block */
    const uint32_t N = (uint32_t)in.size();
    std::vector<Ask> asks;
    const uint32_t wins[][2] = {{0, 0}, {1, 1}, {3, 0}, {0, 3}, {ALL, ALL}, {ALL, 0}, {2, ALL}};
    uint32_t w = 0;
    for (uint32_t cap : {ALL, 0u, 1u, 63u, 64u, 65u, 257u}) {
        asks.push_back(Ask{{0x61}, 0, cap, wins[w % 7][0], wins[w % 7][1]}), ++w;
        asks.push_back(Ask{{0x61, 0x61}, 0, cap, wins[w % 7][0], wins[w % 7][1]}), ++w;
    }
    for (auto& win : wins) {
        asks.push_back(Ask{{0x61, 0x62}, 0, ALL, win[0], win[1]});
        asks.push_back(Ask{{0x62, 0x41, 0x42}, PTX_FIND_ASCII_NOCASE, 5, win[0], win[1]}); /* "bAB" folded: "bab", "b" + "ab", ... */
    }
    asks.push_back(Ask{{0x4E00, 0x4E01}, 0, ALL, 1, 1}); /* inside the long value: hit_end == hit_start + 1 */
    asks.push_back(Ask{{0x7A}, 0, ALL, 1, 1});           /* no hit anywhere */
    bad |= run(t, in, 0, N, asks, "whole batch");
    bad |= run(t, in, 5, N - 7, asks, "a range behind log 0");
    bad |= run(t, in, N - 1, 1, asks, "the dense log alone");
    bad |= run(t, in, N - 3, 1, asks, "the failed log alone");
    bad |= run(t, in, 4, 0, asks, "the empty view");
    if (bad) return 1;
    printf("view emulation ok\n");
    return 0;
}
