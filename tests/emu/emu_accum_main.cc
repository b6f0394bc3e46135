/*
 * Stand-alone sanitizer program of the accumulate emulation — TEST TOOLING ONLY (tests/test_emu_accum.py compiles it with g++ -fsanitize=address,undefined
 * and runs it as a child process).  It builds patch streams itself — inserts, deletes of up to three characters and marks of all four types at and around the
 * 64-character chunk edges, inserts that carry comment ids — runs accum_core.h through emu_accum.cc with both state stores in the three lane orders, and
 * checks rows, counts and digests against the sequential model below; then one malformed record per kind of error.  Every block (LDS, state slice, output
 * rows of the last log) is exactly as large as the host library makes it, so a store past its end is the sanitizer's to report.
 */
#include "emu_accum.cc"

#include <stdio.h>

#include <set>
#include <vector>

struct Chr {
    uint32_t val, attr;
    std::set<uint32_t> ids;
};
struct Log {
    std::vector<uint32_t> payload;
    std::vector<uint8_t> action, mark_type;
    std::vector<ptx_patch> recs;
    uint32_t n_ins = 0, n_ids = 0;
};
struct Want {
    uint32_t status = 0, bad = 0xFFFFFFFFu, n_elems = 0;
    std::vector<uint32_t> values;
    std::vector<ptx_span> spans;
    std::vector<ptx_cinterval> cints;
    uint64_t h1 = 0, h2 = 0;
};

static uint32_t g_rng = 12345u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return n ? (g_rng >> 8) % n : 0u;
}

/* the sequential model: tests/helpers.py accumulate_patches at id level, with the statuses of include/peritext_hip.h */
static Want model(const Log& lg) {
    Want w;
    std::vector<Chr> doc;
    const uint32_t N = (uint32_t)lg.payload.size();
    bool after_insert = false;
    size_t last = 0;
    for (uint32_t k = 0; k < lg.recs.size(); ++k) {
        const ptx_patch& r = lg.recs[k];
        uint32_t err = 0;
        const bool mark = r.kind == PTX_PATCH_ADDMARK || r.kind == PTX_PATCH_REMOVEMARK;
        if (r.kind > 5u || r.row >= N) err = PTX_ERR_BAD_OP;
        else if (r.kind == PTX_PATCH_INSERT_COMMENT && (!after_insert || r.a >= lg.n_ids)) err = PTX_ERR_BAD_OP;
        else if (mark && ((lg.action[r.row] != PTX_ACT_ADDMARK && lg.action[r.row] != PTX_ACT_REMOVEMARK) || lg.mark_type[r.row] > 3 ||
                          (lg.mark_type[r.row] == PTX_MARK_COMMENT && lg.payload[r.row] >= lg.n_ids)))
            err = PTX_ERR_BAD_OP;
        else if (r.kind == PTX_PATCH_INSERT && r.a > doc.size()) err = PTX_ERR_INDEX_OOB;
        else if (r.kind == PTX_PATCH_DELETE && (uint64_t)r.a + r.b > doc.size()) err = PTX_ERR_INDEX_OOB;
        else if (mark && (r.b > doc.size() || r.a > r.b)) err = PTX_ERR_INDEX_OOB;
        else if (r.kind == PTX_PATCH_INSERT && w.n_elems >= lg.n_ins) err = PTX_ERR_CAPACITY;
        if (err) {
            Want f;
            f.status = err, f.bad = k;
            return f;
        }
        if (r.kind == PTX_PATCH_INSERT) {
            Chr c;
            c.val = lg.payload[r.row], c.attr = r.b;
            doc.insert(doc.begin() + r.a, c);
            last = r.a;
            w.n_elems += 1;
        } else if (r.kind == PTX_PATCH_INSERT_COMMENT) {
            doc[last].ids.insert(r.a);
        } else if (r.kind == PTX_PATCH_DELETE) {
            doc.erase(doc.begin() + r.a, doc.begin() + r.a + r.b);
        } else if (mark) {
            const bool add = r.kind == PTX_PATCH_ADDMARK;
            const uint32_t mt = lg.mark_type[r.row], pay = lg.payload[r.row];
            for (uint32_t i = r.a; i < r.b; ++i) {
                Chr& c = doc[i];
                if (mt == PTX_MARK_STRONG) c.attr = add ? c.attr | PTX_ATTR_STRONG : c.attr & ~PTX_ATTR_STRONG;
                else if (mt == PTX_MARK_EM) c.attr = add ? c.attr | PTX_ATTR_EM : c.attr & ~PTX_ATTR_EM;
                else if (mt == PTX_MARK_LINK) c.attr = add ? (c.attr & ~PTX_ATTR_ID_MASK) | PTX_ATTR_LINK | (pay & PTX_ATTR_ID_MASK) : c.attr & ~(PTX_ATTR_LINK | PTX_ATTR_ID_MASK);
                else {
                    c.attr |= PTX_ATTR_COMMENT;
                    if (add) c.ids.insert(pay);
                    else c.ids.erase(pay);
                }
            }
        }
        after_insert = r.kind == PTX_PATCH_INSERT || r.kind == PTX_PATCH_INSERT_COMMENT;
    }
    for (uint32_t i = 0; i < doc.size(); ++i) {
        w.values.push_back(doc[i].val);
        if (i == 0 || doc[i].attr != doc[i - 1].attr || doc[i].ids != doc[i - 1].ids) w.spans.push_back(ptx_span{i, doc[i].attr});
    }
    for (uint32_t c = 0; c < lg.n_ids; ++c)
        for (uint32_t i = 0; i < doc.size(); ++i)
            if (doc[i].ids.count(c) && (i == 0 || !doc[i - 1].ids.count(c))) {
                uint32_t e = i;
                while (e < doc.size() && doc[e].ids.count(c)) ++e;
                w.cints.push_back(ptx_cinterval{c, i, e});
            }
    for (uint32_t i = 0; i < w.values.size(); ++i) ptx_digest_item(w.h1, w.h2, 1u, i, w.values[i], 0u);
    for (uint32_t i = 0; i < w.spans.size(); ++i) ptx_digest_item(w.h1, w.h2, 2u, i, w.spans[i].start, w.spans[i].attr);
    for (const ptx_cinterval& ci : w.cints) ptx_digest_item(w.h1, w.h2, 3u, ci.id, ci.start, ci.end);
    ptx_digest_item(w.h1, w.h2, 4u, 0u, (uint32_t)w.values.size(), (uint32_t)w.spans.size());
    ptx_digest_item(w.h1, w.h2, 4u, 1u, (uint32_t)w.cints.size(), w.n_elems);
    return w;
}

/* a stream of `steps` records over a text that starts with `first` characters: a row per record */
static Log make_log(uint32_t first, uint32_t steps, uint32_t n_ids) {
    Log lg;
    lg.n_ids = n_ids;
    auto row = [&](uint8_t act, uint8_t mt, uint32_t pay) {
        lg.action.push_back(act), lg.mark_type.push_back(mt), lg.payload.push_back(pay);
        return (uint32_t)lg.payload.size() - 1u;
    };
    lg.recs.push_back(ptx_patch{row(PTX_ACT_MAKELIST, 0, 0), PTX_PATCH_MAKELIST, 0, 0});
    uint32_t len = 0;
    static const uint32_t edges[] = {0, 1, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193};
    auto pos = [&](uint32_t lim) { /* an index <= lim, drawn towards the chunk edges */
        const uint32_t e = edges[rnd(13)];
        return rnd(3) && e <= lim ? e : rnd(lim + 1);
    };
    auto insert = [&](uint32_t at) {
        uint32_t attr = rnd(4) == 0 ? (rnd(2) ? PTX_ATTR_STRONG : PTX_ATTR_LINK | rnd(5)) : 0u;
        const uint32_t nc = n_ids && rnd(5) == 0 ? 1 + rnd(n_ids < 3 ? n_ids : 3) : 0;
        if (nc) attr |= PTX_ATTR_COMMENT;
        const uint32_t r = row(PTX_ACT_INSERT, 0, 1000 + rnd(50));
        lg.recs.push_back(ptx_patch{r, PTX_PATCH_INSERT, at, attr});
        for (uint32_t j = 0; j < nc; ++j) lg.recs.push_back(ptx_patch{r, PTX_PATCH_INSERT_COMMENT, (rnd(n_ids) + j) % n_ids, 0});
        lg.n_ins += 1, len += 1;
    };
    for (uint32_t i = 0; i < first; ++i) insert(rnd(2) ? len : pos(len));
    for (uint32_t s = 0; s < steps; ++s) {
        const uint32_t what = rnd(10);
        if (what < 3) insert(pos(len));
        else if (what < 5 && len) {
            const uint32_t a = pos(len - 1), b = 1 + rnd(len - a < 3 ? len - a : 3);
            lg.recs.push_back(ptx_patch{row(PTX_ACT_DELETE, 0, 0), PTX_PATCH_DELETE, a, b});
            len -= b;
        } else {
            const uint32_t a = pos(len), b = rnd(6) == 0 ? a : a + rnd(len - a + 1), mt = n_ids ? rnd(4) : (rnd(3) == 2 ? 3 : rnd(2));
            const bool add = rnd(3) != 0;
            const uint32_t pay = mt == PTX_MARK_COMMENT ? rnd(n_ids) : mt == PTX_MARK_LINK ? rnd(5) : 0;
            lg.recs.push_back(ptx_patch{row(add ? PTX_ACT_ADDMARK : PTX_ACT_REMOVEMARK, (uint8_t)mt, pay), add ? PTX_PATCH_ADDMARK : PTX_PATCH_REMOVEMARK, a, b});
        }
    }
    return lg;
}

static int run(const std::vector<Log>& logs, const char* what) {
    const uint32_t L = (uint32_t)logs.size();
    std::vector<uint64_t> off(1, 0), poff(1, 0);
    std::vector<uint32_t> payload;
    std::vector<uint8_t> action, mark_type;
    std::vector<ptx_patch> recs;
    std::vector<ptx_patch_log> plogs;
    std::vector<ptx_log_hdr> hdr(L);
    for (uint32_t l = 0; l < L; ++l) {
        const Log& g = logs[l];
        payload.insert(payload.end(), g.payload.begin(), g.payload.end());
        action.insert(action.end(), g.action.begin(), g.action.end());
        mark_type.insert(mark_type.end(), g.mark_type.begin(), g.mark_type.end());
        recs.insert(recs.end(), g.recs.begin(), g.recs.end());
        off.push_back(payload.size()), poff.push_back(recs.size());
        plogs.push_back(ptx_patch_log{PTX_OK, (uint32_t)g.recs.size()});
        memset(&hdr[l], 0, sizeof(ptx_log_hdr));
        hdr[l].n_ins = g.n_ins, hdr[l].n_comment_ids = g.n_ids;
    }
    ptx_batch b;
    memset(&b, 0, sizeof(b));
    b.n_logs = L, b.n_ops = payload.size(), b.log_off = off.data(), b.payload = payload.data(), b.action = action.data(), b.mark_type = mark_type.data(), b.log_hdr = hdr.data();
    int fails = 0;
    for (int hbm = 0; hbm < 2; ++hbm)
        for (int reverse = 0; reverse < 3; ++reverse) {
            std::vector<ptx_log_result> res(L);
            std::vector<uint32_t> values(payload.size());
            std::vector<ptx_span> spans(payload.size());
            std::vector<ptx_cinterval> cints(payload.size());
            if (ptx_emu_accum(&b, poff.data(), plogs.data(), recs.data(), res.data(), values.data(), spans.data(), cints.data(), nullptr, nullptr, hbm, reverse, 160 * 1024, nullptr)) return 1;
            for (uint32_t l = 0; l < L; ++l) {
                const Want w = model(logs[l]);
                const ptx_log_result& r = res[l];
                bool ok = r.status == w.status && r.reserved[1] == w.bad;
                if (w.status == PTX_OK) {
                    ok = ok && r.n_elems == w.n_elems && r.n_visible == w.values.size() && r.n_spans == w.spans.size() && r.n_cintervals == w.cints.size() && r.digest[0] == w.h1 &&
                         r.digest[1] == w.h2;
                    for (uint32_t i = 0; ok && i < w.values.size(); ++i) ok = values[off[l] + i] == w.values[i];
                    for (uint32_t i = 0; ok && i < w.spans.size(); ++i) ok = spans[off[l] + i].start == w.spans[i].start && spans[off[l] + i].attr == w.spans[i].attr;
                    for (uint32_t i = 0; ok && i < w.cints.size(); ++i)
                        ok = cints[off[l] + i].id == w.cints[i].id && cints[off[l] + i].start == w.cints[i].start && cints[off[l] + i].end == w.cints[i].end;
                } else {
                    ok = ok && r.n_visible == 0 && r.n_spans == 0 && r.n_cintervals == 0 && r.digest[0] == 0 && r.digest[1] == 0;
                }
                if (!ok) {
                    printf("%s: log %u differs (store %d, lane order %d): status %u / %u, bad record %u / %u, visible %u / %zu, spans %u / %zu, intervals %u / %zu\n", what, l, hbm, reverse,
                           r.status, w.status, r.reserved[1], w.bad, r.n_visible, w.values.size(), r.n_spans, w.spans.size(), r.n_cintervals, w.cints.size());
                    ++fails;
                }
            }
        }
    return fails;
}

int main() {
    int fails = 0;
    /* well-formed streams: texts below, at and beyond one, two and three chunks; none, one, and 40 comment ids (more than one bitmap word per row at 200 characters) */
    std::vector<Log> logs;
    const uint32_t firsts[] = {0, 1, 63, 64, 65, 127, 128, 129, 130, 200};
    for (uint32_t f : firsts)
        for (uint32_t ids : {0u, 1u, 40u}) logs.push_back(make_log(f, 150, ids));
    logs.push_back(make_log(0, 0, 0)); /* the empty document */
    fails += run(logs, "well-formed");
    uint32_t well = 0;
    for (const Log& g : logs) well += model(g).status == PTX_OK;
    if (well != logs.size()) printf("a generated stream is malformed\n"), ++fails;

    /* one malformed record each, beside a good neighbour */
    const Log good = make_log(130, 120, 5);
    std::vector<uint32_t> len_before;
    uint32_t len = 0;
    for (const ptx_patch& r : good.recs) {
        len_before.push_back(len);
        len += r.kind == PTX_PATCH_INSERT ? 1u : 0u;
        len -= r.kind == PTX_PATCH_DELETE ? r.b : 0u;
    }
    auto last_of = [&](uint32_t kind) {
        uint32_t k = 0;
        for (uint32_t i = 0; i < good.recs.size(); ++i)
            if (good.recs[i].kind == kind) k = i;
        return k;
    };
    const uint32_t ki = last_of(PTX_PATCH_INSERT), kd = last_of(PTX_PATCH_DELETE), km = last_of(PTX_PATCH_ADDMARK), kc = last_of(PTX_PATCH_INSERT_COMMENT);
    std::vector<Log> bad;
    auto tamper = [&](uint32_t k, uint32_t ptx_patch::*field, uint32_t v) {
        Log g = good;
        g.recs[k].*field = v;
        bad.push_back(g);
        bad.push_back(good);
    };
    tamper(ki, &ptx_patch::a, len_before[ki] + 1u);
    tamper(kd, &ptx_patch::a, len_before[kd]);
    tamper(kd, &ptx_patch::b, 0xFFFFFFFFu); /* a + b wraps in 32 bits */
    tamper(km, &ptx_patch::b, len_before[km] + 1u);
    tamper(km, &ptx_patch::a, good.recs[km].b + 1u);
    tamper(km, &ptx_patch::a, 0xFFFFFFF0u);
    tamper(km, &ptx_patch::kind, 9u);
    {
        Log g = good; /* an INSERT_COMMENT of a valid id behind a record that is no insert */
        uint32_t ko = 0;
        for (uint32_t i = 1; i < good.recs.size(); ++i)
            if (good.recs[i].kind == PTX_PATCH_ADDMARK && good.recs[i - 1].kind != PTX_PATCH_INSERT && good.recs[i - 1].kind != PTX_PATCH_INSERT_COMMENT) ko = i;
        g.recs[ko].kind = PTX_PATCH_INSERT_COMMENT, g.recs[ko].a = 0;
        bad.push_back(g);
        bad.push_back(good);
    }
    tamper(kd, &ptx_patch::row, (uint32_t)good.payload.size());
    tamper(kd, &ptx_patch::row, 0xFFFFFFFFu);
    tamper(kc, &ptx_patch::a, good.n_ids);
    tamper(km, &ptx_patch::row, good.recs[kd].row); /* a mark record whose row is a delete */
    {
        Log g = good; /* one INSERT record more than the log has insert rows */
        g.recs.push_back(ptx_patch{good.recs[ki].row, PTX_PATCH_INSERT, 0, 0});
        bad.push_back(g);
        bad.push_back(good);
    }
    uint32_t n_bad = 0;
    for (const Log& g : bad) n_bad += model(g).status != PTX_OK;
    if (n_bad != 13) printf("%u of 13 tampered streams are malformed for the model\n", n_bad), ++fails;
    fails += run(bad, "malformed");
    if (fails) {
        printf("accum emulation FAILED: %d\n", fails);
        return 1;
    }
    printf("accum emulation ok: %zu well-formed and %zu tampered streams, two stores, three lane orders\n", logs.size(), bad.size() / 2);
    return 0;
}
