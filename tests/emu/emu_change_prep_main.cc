/*
 * Stand-alone sanitizer program of the change-preparation emulation — TEST TOOLING ONLY (tests/test_emu_change_prep.py compiles it with g++
 * -fsanitize=address,undefined and runs it as a child process).  It builds InputOperations and base headers itself — logs of 0, 1, 63, 64, 65, 128 and 129 ops,
 * logs of 0 to 3 Changes, random mixes of every action, inserts that end exactly at n_values and one past it, rows at and above the limit, offsets that
 * decrease — and runs the offsets check, the prepare pass and the scans through emu_change_prep.cc in the three lane orders, against the sequential loop below
 * (ptx_change's own, restated).  Every array is a heap block of exactly the size the library is given — chg_off ends at entry n_logs, op_off at entry n_changes,
 * the op columns at the last op, the outputs at their last word — so a read of op 64 of a log of 64, or a store one log too far, is the sanitizer's finding.
 */
#include "emu_change_prep.cc"

#include <stdio.h>

#include <vector>

static uint32_t g_rng = 90217u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

template <class T>
static T* exact(const std::vector<T>& v) { /* a block that ends at the last element */
    T* p = (T*)malloc(v.size() * sizeof(T) ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Case {
    std::vector<uint64_t> chg_off, op_off, log_off;
    std::vector<uint8_t> action;
    std::vector<uint32_t> count, payload;
    std::vector<ptx_log_hdr> hdr;
    uint64_t n_values = 0;
    uint32_t has_values = 1, max_actors = 3, all_in_hbm = 0;
    uint64_t max_lds = 160 * 1024;
    /* sizes as the object is made with: by default what the offsets end at */
    bool sizes_given = false;
    uint64_t n_changes = 0, n_input_ops = 0;
};

/* ptx_change's host walk: 0 or the first error in ITS order, and the per-log figures */
static uint64_t sequential(const Case& c, std::vector<uint32_t>& rows, std::vector<uint32_t>& lw, uint64_t& need) {
    const uint32_t L = (uint32_t)c.hdr.size();
    const uint64_t NC = c.n_changes, NI = c.n_input_ops;
    uint64_t err = PTX_CP_NO_ERROR;
    auto note = [&](uint64_t w) {
        if (w < err) err = w;
    };
    rows.assign(L, 0);
    lw.assign(L, 0);
    need = 0;
    if (!L) return err;
    if (c.chg_off[0] != 0) note(PTX_CP_WORD(PTX_CP_CHG_START, 0));
    for (uint32_t l = 0; l < L; ++l)
        if (c.chg_off[l + 1] < c.chg_off[l]) note(PTX_CP_WORD(PTX_CP_CHG_ORDER, l + 1));
    if (c.chg_off[L] != NC) note(PTX_CP_WORD(PTX_CP_SIZES, 0));
    if (NC) {
        if (c.op_off[0] != 0) note(PTX_CP_WORD(PTX_CP_OP_START, 0));
        for (uint64_t k = 0; k < NC; ++k)
            if (c.op_off[k + 1] < c.op_off[k]) note(PTX_CP_WORD(PTX_CP_OP_ORDER, k + 1));
        if (c.op_off[NC] != NI) note(PTX_CP_WORD(PTX_CP_SIZES, 1));
    }
    if (err != PTX_CP_NO_ERROR) return err; /* (the per-log figures of a call with bad offsets are nobody's to read) */
    for (uint32_t l = 0; l < L; ++l) {
        if (c.chg_off[l + 1] == c.chg_off[l]) continue;
        uint64_t r = 0, g = 0;
        bool bad = false;
        for (uint64_t q = c.op_off[c.chg_off[l]]; q < c.op_off[c.chg_off[l + 1]]; ++q) {
            if (c.action[q] == PTX_IN_INSERT) {
                if ((uint64_t)c.payload[q] + c.count[q] > c.n_values || (c.count[q] && !c.has_values)) bad = true;
                r += c.count[q], g += c.count[q];
            } else if (c.action[q] == PTX_IN_DELETE) r += c.count[q];
            else r += 1;
        }
        if (bad) note(PTX_CP_WORD(PTX_CP_VALUES, l));
        if (r > PTX_CHANGE_ROWS_MAX) note(PTX_CP_WORD(PTX_CP_ROWS, l));
        if (bad || r > PTX_CHANGE_ROWS_MAX) continue;
        const bool has_rows = c.log_off[l + 1] > c.log_off[l];
        const uint64_t n = has_rows ? c.hdr[l].n_ins : 0;
        const bool in_hbm = c.all_in_hbm || ptx_change_lds_need(n, g, 1, c.max_actors) > c.max_lds;
        rows[l] = (uint32_t)r;
        lw[l] = in_hbm ? (uint32_t)ptx_change_list_words(n, g) : 0u;
        const uint64_t nd = ptx_change_lds_need(n, g, 1, c.max_actors, in_hbm);
        if (nd > need) need = nd;
    }
    return err;
}

static int run(Case c, const char* what) {
    const uint32_t L = (uint32_t)c.hdr.size();
    if (!c.sizes_given) {
        c.n_changes = L ? c.chg_off[L] : 0;
        c.n_input_ops = c.n_changes ? c.op_off[c.n_changes] : 0;
    }
    std::vector<uint32_t> want_rows, want_lw;
    uint64_t want_need = 0;
    const uint64_t want_err = sequential(c, want_rows, want_lw, want_need);
    uint64_t* chg_off = exact(c.chg_off);
    uint64_t* op_off = exact(c.op_off);
    uint64_t* log_off = exact(c.log_off);
    uint8_t* action = exact(c.action);
    uint32_t* count = exact(c.count);
    uint32_t* payload = exact(c.payload);
    ptx_log_hdr* hdr = exact(c.hdr);
    EmuPrepIn in;
    memset(&in, 0, sizeof(in));
    in.chg_off = chg_off, in.op_off = op_off, in.action = action, in.count = count, in.payload = payload;
    in.n_changes = c.n_changes, in.n_input_ops = c.n_input_ops, in.n_values = c.n_values, in.has_values = c.has_values, in.n_logs = L;
    in.log_off = log_off, in.log_hdr = hdr, in.max_actors = c.max_actors, in.all_in_hbm = c.all_in_hbm, in.max_lds = c.max_lds;
    int bad = 0;
    for (int rev = 0; rev < 3 && !bad; ++rev) {
        uint32_t* rows = (uint32_t*)malloc(L ? L * 4 : 1);
        uint32_t* lw = (uint32_t*)malloc(L ? L * 4 : 1);
        uint64_t* out_off = (uint64_t*)malloc(((size_t)L + 1) * 8);
        uint64_t* list_off = (uint64_t*)malloc(((size_t)L + 1) * 8);
        memset(rows, 0xA5, L * 4), memset(lw, 0xA5, L * 4), memset(out_off, 0xA5, ((size_t)L + 1) * 8), memset(list_off, 0xA5, ((size_t)L + 1) * 8);
        uint64_t err = 0, need = 0;
        if (ptx_emu_change_prep(&in, rev, rows, lw, out_off, list_off, &err, &need) != 0) bad = 1;
        if (err != want_err) bad = 2;
        if (!bad && err == PTX_CP_NO_ERROR) {
            uint64_t ro = 0, lo = 0;
            if (need != want_need) bad = 3;
            for (uint32_t l = 0; l < L && !bad; ++l) {
                if (rows[l] != want_rows[l] || lw[l] != want_lw[l] || out_off[l] != ro || list_off[l] != lo) bad = 4;
                ro += want_rows[l], lo += want_lw[l];
            }
            if (!bad && (out_off[L] != ro || list_off[L] != lo)) bad = 5;
        }
        if (bad) printf("FAIL %s: order %d, check %d (err %llx, want %llx)\n", what, rev, bad, (unsigned long long)err, (unsigned long long)want_err);
        free(rows), free(lw), free(out_off), free(list_off);
    }
    free(chg_off), free(op_off), free(log_off), free(action), free(count), free(payload), free(hdr);
    return bad;
}

/* a batch whose log l makes changes[l] Changes of the given op counts (spread over them), random actions */
static Case build(const std::vector<uint32_t>& n_changes_of, const std::vector<uint32_t>& n_ops_of, uint64_t n_values) {
    Case c;
    const uint32_t L = (uint32_t)n_changes_of.size();
    c.n_values = n_values;
    c.chg_off.push_back(0), c.op_off.push_back(0), c.log_off.push_back(0);
    for (uint32_t l = 0; l < L; ++l) {
        ptx_log_hdr h;
        memset(&h, 0, sizeof(h));
        const uint32_t n_rows = l % 5 == 4 ? 0 : 1 + rnd(300);
        h.n_ins = n_rows ? rnd(n_rows) : 0;
        h.max_counter = n_rows, h.max_actor = rnd(3);
        c.hdr.push_back(h);
        c.log_off.push_back(c.log_off.back() + n_rows);
        uint32_t left = n_changes_of[l] ? n_ops_of[l] : 0;
        for (uint32_t k = 0; k < n_changes_of[l]; ++k) {
            const uint32_t take = k + 1 == n_changes_of[l] ? left : (k == 0 ? 0 : rnd(left + 1)); /* (the first of several Changes has no ops) */
            left -= take;
            for (uint32_t j = 0; j < take; ++j) {
                const uint8_t a = (uint8_t)rnd(7);
                c.action.push_back(a);
                const uint32_t cnt = rnd(6);
                c.count.push_back(cnt);
                c.payload.push_back(a == PTX_IN_INSERT ? (n_values >= cnt ? rnd((uint32_t)(n_values - cnt) + 1) : 0) : rnd(1000));
            }
            c.op_off.push_back(c.op_off.back() + take);
        }
        c.chg_off.push_back(c.chg_off.back() + n_changes_of[l]);
    }
    return c;
}

int main() {
    int failed = 0;
    /* the lane edges: one log of each length; 0 to 3 Changes */
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 128u, 129u})
        for (uint32_t ch : {1u, 2u, 3u}) failed += run(build({0, ch, 0, 1}, {0, n, 0, 1}, 40), "lane edges") != 0;
    failed += run(build({}, {}, 0), "no logs") != 0;
    failed += run(build({0, 0, 0}, {0, 0, 0}, 0), "no changes") != 0;
    /* many logs, most of them idle: the scan's chunk edges */
    for (uint32_t L : {1u, 1023u, 1024u, 1025u, 2049u}) {
        std::vector<uint32_t> ch(L, 0), no(L, 0);
        for (uint32_t l = 0; l < L; l += 1 + rnd(97)) ch[l] = 1 + rnd(3), no[l] = rnd(70);
        ch[L - 1] = 1, no[L - 1] = 3;
        Case c = build(ch, no, 25);
        failed += run(c, "many logs") != 0;
        c.all_in_hbm = 1;
        failed += run(c, "many logs, lists in HBM") != 0;
        c.all_in_hbm = 0, c.max_lds = 600; /* some lists fit, some do not */
        failed += run(c, "many logs, a small LDS") != 0;
    }
    /* the limits */
    auto one = [](uint8_t a, uint32_t cnt, uint32_t pay, uint64_t nv) {
        Case c = build({1}, {0}, nv);
        c.action = {a}, c.count = {cnt}, c.payload = {pay};
        c.op_off = {0, 1};
        return c;
    };
    failed += run(one(PTX_IN_DELETE, 65534, 0, 0), "65534 rows") != 0;
    failed += run(one(PTX_IN_DELETE, 65535, 0, 0), "65535 rows") != 0;
    failed += run(one(PTX_IN_INSERT, 7, 3, 10), "insert ends at n_values") != 0;
    failed += run(one(PTX_IN_INSERT, 8, 3, 10), "insert ends behind n_values") != 0;
    failed += run(one(PTX_IN_INSERT, 2, 0xFFFFFFFFu, 10), "payload + count wraps in 32 bits") != 0;
    {
        Case c = one(PTX_IN_INSERT, 0, 0, 0);
        c.has_values = 0;
        failed += run(c, "zero-count insert, no values") != 0;
        c.count = {1}, c.n_values = 5;
        failed += run(c, "insert, no values") != 0;
    }
    {
        Case c = build({0, 1, 1}, {0, 65, 65}, 0);
        for (auto& a : c.action) a = PTX_IN_DELETE;
        for (auto& n : c.count) n = 1008;
        c.count[64] = 1022; /* 64 * 1008 + 1022 = 65534 */
        failed += run(c, "65534 rows of 65 ops") != 0;
        c.count[129] = 1023; /* the last op of the second log tips it */
        failed += run(c, "65535 rows of 65 ops") != 0;
        c.count[64] = 1023; /* both: the lower log is reported */
        failed += run(c, "two logs over the limit") != 0;
    }
    /* offsets */
    for (uint32_t at : {1u, 255u, 256u, 257u, 600u}) {
        std::vector<uint32_t> ch(600, 1), no(600, 2);
        Case c = build(ch, no, 9);
        c.sizes_given = true, c.n_changes = 600, c.n_input_ops = 1200;
        Case d = c;
        c.chg_off[at] = at == 1 ? 0 : c.chg_off[at - 1] - 1;
        if (at == 1) c.chg_off[0] = 0, c.chg_off[1] = 2, c.chg_off[2] = 1;
        failed += run(c, "chg_off decreases") != 0;
        d.op_off[at] = d.op_off[at - 1] - (at == 1 ? 0 : 1);
        if (at == 1) d.op_off[1] = 5, d.op_off[2] = 4;
        failed += run(d, "op_off decreases") != 0;
    }
    {
        Case c = build({1, 1}, {2, 2}, 9);
        c.sizes_given = true, c.n_changes = 2, c.n_input_ops = 4;
        Case d = c, e = c;
        c.chg_off[0] = 1;
        failed += run(c, "chg_off starts at 1") != 0;
        d.op_off[0] = 1;
        failed += run(d, "op_off starts at 1") != 0;
        e.n_input_ops = 3;
        e.action.pop_back(), e.count.pop_back(), e.payload.pop_back(); /* columns of three ops under offsets that name four: nothing is read behind them */
        failed += run(e, "op_off ends behind the columns") != 0;
    }
    if (failed) {
        printf("%d cases failed\n", failed);
        return 1;
    }
    printf("change prep emulation ok\n");
    return 0;
}
