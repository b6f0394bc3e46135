/*
 * Stand-alone sanitizer program of the mark-run emulation — TEST TOOLING ONLY (tests/test_emu_markruns.py compiles it with g++ -fsanitize=address,undefined and runs
 * it as a child process).  It builds a string table and merge results itself — logs of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 200 span rows with strong, em and
 * links of a few urls (one of them PTX_ATTR_ID_MASK) drawn at random, 0, 63, 64 and 65 comment intervals of three ids in the result's (id, start) order, values of
 * 0, 1 and 3 units, a failed log between good ones — makes a view through emu_view.cc, then runs count, emit, finish with windows and the hit filter in the three
 * lane orders for every selector under several caps, and compares with the sequential walks below.  Every buffer is exactly as large as the library makes it: the
 * span rows and the comment intervals end at the last row of the last log, the per-run arrays at the last listed run, the kept hits at the last listed hit — so a
 * neighbour read one row past a log's last, or a store one run too far, is the sanitizer's finding.
 */
#include "emu_markruns.cc"

#include <stdio.h>

#include <algorithm>
#include <vector>

static uint32_t g_rng = 1848u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

struct LogIn {
    uint32_t status;
    std::vector<uint32_t> ids;
    std::vector<ptx_span> spans;
    std::vector<ptx_cinterval> cints;
};

struct Run {
    uint32_t s, e, id;
};

static bool row_match(uint32_t mt, uint32_t id, uint32_t attr) {
    if (mt == PTX_MARK_STRONG) return attr & PTX_ATTR_STRONG;
    if (mt == PTX_MARK_EM) return attr & PTX_ATTR_EM;
    return (attr & PTX_ATTR_LINK) && (id == PTX_MARK_ANY_ID || (attr & PTX_ATTR_ID_MASK) == id);
}

/* the sequential answer: one row after the other, an open run in hand */
static std::vector<Run> seq_runs(const LogIn& g, uint32_t mt, uint32_t id) {
    std::vector<Run> out;
    if (g.status != PTX_OK) return out;
    const uint32_t nv = (uint32_t)g.ids.size();
    if (mt == PTX_MARK_COMMENT) {
        for (const ptx_cinterval& c : g.cints)
            if (id == PTX_MARK_ANY_ID || c.id == id) out.push_back(Run{c.start, c.end, c.id});
        return out;
    }
    bool open = false;
    for (size_t i = 0; i < g.spans.size(); ++i) {
        const uint32_t at = g.spans[i].attr, key = mt == PTX_MARK_LINK ? at & PTX_ATTR_ID_MASK : 0u;
        const bool m = row_match(mt, id, at);
        if (open && (!m || key != out.back().id)) out.back().e = g.spans[i].start, open = false;
        if (m && !open) out.push_back(Run{g.spans[i].start, nv, key}), open = true;
    }
    return out;
}

static LogIn make_log(uint32_t rows, uint32_t n_cints, const uint32_t* urls) {
    LogIn g;
    g.status = PTX_OK;
    uint32_t at = 0;
    for (uint32_t r = 0; r < rows; ++r) {
        uint32_t attr = 0;
        if (rnd(3) == 0) attr |= PTX_ATTR_STRONG;
        if (r & 1u) attr |= PTX_ATTR_EM; /* (a row differs from its neighbour) */
        if (rnd(2) == 0) attr |= PTX_ATTR_LINK | urls[rnd(3)];
        g.spans.push_back(ptx_span{at, attr});
        at += 1u + rnd(3);
    }
    for (uint32_t e = 0; e < at; ++e) g.ids.push_back(rnd(3)); /* strings of 0, 1 and 3 units */
    const uint32_t per = n_cints / 3u, nv = at;
    for (uint32_t id = 0; id < 3u && nv; ++id) { /* (id, start): every id starts over at the front */
        const uint32_t n = id == 1u ? n_cints - 2u * per : per;
        for (uint32_t k = 0; k < n && 2u * k + 1u <= nv; ++k) g.cints.push_back(ptx_cinterval{id + 4u, 2u * k, 2u * k + 1u});
    }
    return g;
}

static int check(const std::vector<LogIn>& in, const char* what) {
    const uint32_t L = (uint32_t)in.size();
    std::vector<uint16_t> units = {0x61, 0x62, 0x63, 0x64};
    std::vector<uint64_t> str_off = {0, 0, 1, 4};
    std::vector<ptx_log_result> logs(L);
    memset(logs.data(), 0, L * sizeof(ptx_log_result));
    std::vector<uint64_t> log_off(L + 1, 0);
    uint64_t span_end = 0, cint_end = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const size_t cap = std::max(in[l].ids.size(), std::max(in[l].spans.size(), in[l].cints.size()));
        log_off[l + 1] = log_off[l] + cap + (l + 1 < L ? 3 : 0);
        if (in[l].status == PTX_OK) span_end = log_off[l] + in[l].spans.size(), cint_end = log_off[l] + in[l].cints.size();
    }
    std::vector<uint32_t> values(log_off[L], 0xDEADBEEFu);
    std::vector<ptx_span> spans(span_end, ptx_span{0xDEADBEEFu, 0xFFFFFFFFu});           /* ends exactly at the last row of the last good log */
    std::vector<ptx_cinterval> cints(cint_end, ptx_cinterval{0xDEADBEEFu, 0u, 0xFFFFFFFFu}); /* ... likewise */
    for (uint32_t l = 0; l < L; ++l) {
        logs[l].status = in[l].status;
        if (in[l].status != PTX_OK) continue;
        logs[l].n_visible = (uint32_t)in[l].ids.size();
        logs[l].n_spans = (uint32_t)in[l].spans.size();
        logs[l].n_cintervals = (uint32_t)in[l].cints.size();
        for (size_t i = 0; i < in[l].ids.size(); ++i) values[log_off[l] + i] = in[l].ids[i];
        for (size_t i = 0; i < in[l].spans.size(); ++i) spans[log_off[l] + i] = in[l].spans[i];
        for (size_t i = 0; i < in[l].cints.size(); ++i) cints[log_off[l] + i] = in[l].cints[i];
    }
    const struct {
        uint32_t mt, id;
    } sels[] = {{PTX_MARK_STRONG, PTX_MARK_ANY_ID}, {PTX_MARK_EM, PTX_MARK_ANY_ID}, {PTX_MARK_LINK, PTX_MARK_ANY_ID}, {PTX_MARK_LINK, 7u}, {PTX_MARK_LINK, PTX_ATTR_ID_MASK},
                {PTX_MARK_LINK, 9u},   {PTX_MARK_COMMENT, PTX_MARK_ANY_ID}, {PTX_MARK_COMMENT, 5u}, {PTX_MARK_COMMENT, 6u}, {PTX_MARK_COMMENT, 99u}};
    const uint32_t caps[] = {0u, 1u, 2u, 64u, 65u, 0xFFFFFFFFu};
    for (int reverse = 0; reverse < 3; ++reverse) {
        EmuView* v = nullptr;
        int rc = ptx_emu_view_create(log_off.data(), L, logs.data(), values.data(), spans.data(), units.data(), str_off.data(), 3u, 0u, L, reverse, &v);
        if (rc != 0) return printf("%s: create rc %d\n", what, rc), 1;
        for (const auto& sel : sels) {
            for (uint32_t cap : caps) {
                std::vector<uint32_t> n_runs(L);
                std::vector<uint64_t> run_off(L + 1);
                rc = ptx_emu_markrun_count(v, cints.data(), logs.data(), sel.mt, sel.id, cap, 0, reverse, n_runs.data(), run_off.data());
                if (rc != 0) return printf("%s: count rc %d\n", what, rc), 1;
                const size_t nr = (size_t)run_off[L];
                std::vector<uint32_t> rs(nr), re(nr), ri(nr), ru(nr), rl(nr), ws(nr), we(nr), mu(nr);
                const uint32_t before = cap & 3u, after = 0xFFFFFFFFu - (cap & 1u);
                rc = ptx_emu_markrun_emit(v, cints.data(), logs.data(), sel.mt, sel.id, cap, reverse, run_off.data(), rs.data(), re.data(), ri.data(), ru.data(), rl.data(), before, after,
                                          ws.data(), we.data(), mu.data());
                if (rc != 0) return printf("%s: emit rc %d\n", what, rc), 1;
                size_t k = 0;
                for (uint32_t l = 0; l < L; ++l) {
                    const std::vector<Run> want = seq_runs(in[l], sel.mt, sel.id);
                    if (n_runs[l] != want.size() || run_off[l] != k)
                        return printf("%s order %d type %u id %u cap %u log %u: %u runs at %llu, want %zu at %zu\n", what, reverse, sel.mt, sel.id, cap, l, n_runs[l],
                                      (unsigned long long)run_off[l], want.size(), k), 1;
                    const uint32_t* pre = v->pre + v->pre_off[l];
                    for (size_t j = 0; j < want.size() && j < cap; ++j, ++k) {
                        const Run& w = want[j];
                        const uint32_t a = w.s > before ? w.s - before : 0u;
                        if (rs[k] != w.s || re[k] != w.e || ri[k] != w.id || ru[k] != pre[w.s] || rl[k] != pre[w.e] - pre[w.s] || ws[k] != a ||
                            we[k] != (w.e > 0xFFFFFFFFu - after ? 0xFFFFFFFFu : w.e + after) || mu[k] != pre[w.s] - pre[a])
                            return printf("%s order %d type %u id %u cap %u log %u run %zu: [%u, %u) id %u, want [%u, %u) id %u\n", what, reverse, sel.mt, sel.id, cap, l, j, rs[k], re[k],
                                          ri[k], w.s, w.e, w.id), 1;
                    }
                }
                if (k != nr) return printf("%s: %zu listed runs, want %zu\n", what, nr, k), 1;
                if (cap != 0xFFFFFFFFu || (sel.mt == PTX_MARK_COMMENT && sel.id == PTX_MARK_ANY_ID)) continue;
                /* the filter over the uncapped runs: hits drawn at random, ascending by start, some inside a run, some over its edge */
                std::vector<uint64_t> hit_off(L + 1, 0);
                std::vector<uint32_t> hu, hs, he;
                for (uint32_t l = 0; l < L; ++l) {
                    const uint32_t nv = in[l].status == PTX_OK ? (uint32_t)in[l].ids.size() : 0u;
                    const uint32_t nh = nv ? (l % 3u == 0u ? 63u + l % 4u : rnd(40)) : 0u;
                    uint32_t s = 0;
                    for (uint32_t h = 0; h < nh && s < nv; ++h) {
                        hu.push_back(s), hs.push_back(s), he.push_back(std::min(nv, s + 1u + rnd(3)));
                        s += rnd(3);
                    }
                    hit_off[l + 1] = hs.size();
                }
                for (uint32_t hcap : caps) {
                    std::vector<uint32_t> n_kept(L);
                    std::vector<uint64_t> out_off(L + 1);
                    ptx_emu_markrun_filter_count(L, hcap, hit_off.data(), hs.data(), he.data(), run_off.data(), rs.data(), re.data(), reverse, n_kept.data(), out_off.data());
                    const size_t nk = (size_t)out_off[L];
                    std::vector<uint32_t> ou(nk), os(nk), oe(nk);
                    ptx_emu_markrun_filter_emit(L, hcap, hit_off.data(), hu.data(), hs.data(), he.data(), run_off.data(), rs.data(), re.data(), reverse, out_off.data(), ou.data(), os.data(),
                                                oe.data());
                    size_t o = 0;
                    for (uint32_t l = 0; l < L; ++l) {
                        uint32_t kept = 0;
                        for (uint64_t h = hit_off[l]; h < hit_off[l + 1]; ++h) {
                            bool in_run = false;
                            for (uint64_t r = run_off[l]; r < run_off[l + 1]; ++r) in_run = in_run || (rs[r] <= hs[h] && he[h] <= re[r]);
                            if (!in_run) continue;
                            if (kept < hcap) {
                                if (o >= nk || ou[o] != hu[h] || os[o] != hs[h] || oe[o] != he[h]) return printf("%s order %d type %u log %u: kept hit %zu differs\n", what, reverse, sel.mt, l, o), 1;
                                ++o;
                            }
                            ++kept;
                        }
                        if (n_kept[l] != kept) return printf("%s order %d type %u id %u log %u: %u kept, want %u\n", what, reverse, sel.mt, sel.id, l, n_kept[l], kept), 1;
                    }
                    if (o != nk) return printf("%s: %zu kept hits listed, want %zu\n", what, nk, o), 1;
                }
            }
        }
        ptx_emu_view_close(v);
    }
    return 0;
}

int main() {
    const uint32_t urls[3] = {7u, 8u, PTX_ATTR_ID_MASK};
    std::vector<LogIn> in;
    const uint32_t rows[] = {0u, 1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 200u};
    const uint32_t cints[] = {0u, 63u, 64u, 65u, 3u, 0u, 190u, 191u, 192u, 195u};
    for (size_t i = 0; i < sizeof(rows) / sizeof(rows[0]); ++i) {
        in.push_back(make_log(rows[i], cints[i], urls));
        if (i == 4) {
            LogIn bad = make_log(10u, 3u, urls); /* a failed log between good ones: it has no runs */
            bad.status = PTX_ERR_SEQ_GAP;
            in.push_back(bad);
        }
    }
    if (check(in, "mixed")) return 1;
    std::vector<LogIn> tail = {make_log(129u, 65u, urls)};
    tail[0].spans.back().attr = PTX_ATTR_STRONG | PTX_ATTR_EM | PTX_ATTR_LINK | PTX_ATTR_ID_MASK; /* every selector's last run reaches the last row: its end is n_visible */
    if (check(tail, "tail")) return 1;
    printf("markrun emulation ok\n");
    return 0;
}
