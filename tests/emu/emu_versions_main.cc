/*
 * Stand-alone sanitizer program of the version-cut emulation — TEST TOOLING ONLY (tests/test_emu_versions.py compiles it with g++ -fsanitize=address,undefined
 * and runs it as a child process).  It generates logs itself (changes of 0 .. 4 ops, 1 .. 17 actors, sizes around the 64-change steps), runs the plan of
 * version_core.h and the gather of sync_core.h through emu_versions.cc in the three lane orders, for clock cuts and prefix cuts, with and without
 * PTX_VERSIONS_THEN_REST, and checks every output against the sequential filter below.
 */
#include "emu_versions.cc"

#include <stdio.h>

#include <vector>

struct Chg {
    uint32_t actor, seq, nops;
    std::vector<uint32_t> deps; /* [na] */
};
struct Log {
    uint32_t na;
    std::vector<Chg> chg;
};
struct Want {
    uint32_t status;
    std::vector<uint32_t> order, clock;
    uint32_t n_kept, first_row;
};

static uint32_t g_rng = 12345u;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

/* a log some replica could have applied: every change depends on what its author had seen of the others so far */
static Log make_log(uint32_t na, uint32_t n) {
    Log l{na, {}};
    std::vector<uint32_t> seq(na, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t a = rnd(na);
        Chg c{a, ++seq[a], rnd(5), std::vector<uint32_t>(na, 0)};
        for (uint32_t b = 0; b < na; ++b)
            if (b != a && seq[b] && rnd(3) == 0) c.deps[b] = 1 + rnd(seq[b]);
        l.chg.push_back(c);
    }
    return l;
}

/* the definition, one change at a time */
static Want filter(const Log& l, const uint32_t* clock, const uint32_t* prefix, bool then_rest) {
    Want w{PTX_OK, {}, std::vector<uint32_t>(l.na, 0), 0, 0};
    std::vector<uint32_t> rest;
    for (uint32_t i = 0; i < l.chg.size(); ++i) {
        const Chg& c = l.chg[i];
        const bool keep = prefix ? i < *prefix : c.seq <= clock[c.actor];
        if (!keep) {
            rest.push_back(i);
            continue;
        }
        if (!prefix)
            for (uint32_t b = 0; b < l.na; ++b)
                if (b != c.actor && c.deps[b] && c.deps[b] > clock[b]) w.status = PTX_ERR_MISSING_DEP;
        w.order.push_back(i);
        w.first_row += c.nops;
        if (c.seq > w.clock[c.actor]) w.clock[c.actor] = c.seq;
    }
    w.n_kept = (uint32_t)w.order.size();
    if (then_rest) w.order.insert(w.order.end(), rest.begin(), rest.end());
    if (w.status != PTX_OK) w = Want{w.status, {}, std::vector<uint32_t>(l.na, 0), 0, 0};
    return w;
}

static int run(const std::vector<Log>& logs, bool use_prefix, bool then_rest, const char* what) {
    uint32_t na = 1;
    for (const Log& l : logs) na = l.na > na ? l.na : na;
    const uint32_t es = PTX_ENV_STRIDE(na), L = (uint32_t)logs.size();
    std::vector<uint64_t> log_off(1, 0), chg_off(1, 0), op_id;
    std::vector<uint32_t> hdr;
    std::vector<uint16_t> env;
    for (uint32_t k = 0; k < L; ++k) {
        for (uint32_t i = 0; i < logs[k].chg.size(); ++i) {
            const Chg& c = logs[k].chg[i];
            hdr.push_back(c.actor << PTX_CHG_ACTOR_SHIFT | c.nops);
            std::vector<uint16_t> row(es, 0);
            row[0] = (uint16_t)c.seq;
            for (uint32_t b = 0; b < logs[k].na; ++b) row[1 + b] = (uint16_t)c.deps[b];
            env.insert(env.end(), row.begin(), row.end());
            for (uint32_t j = 0; j < c.nops; ++j) op_id.push_back(((uint64_t)(100000u * k + 8u * i + j + 1u) << 32) | c.actor); /* the id says where the row came from */
        }
        log_off.push_back(op_id.size());
        chg_off.push_back(hdr.size());
    }
    const size_t T = op_id.size();
    std::vector<uint64_t> zero64(T + 1, 0);
    std::vector<uint32_t> pay(T + 1, 7);
    std::vector<uint8_t> act(T + 1, PTX_ACT_INSERT), zero8(T + 1, 0);
    hdr.push_back(0);
    ptx_batch b;
    memset(&b, 0, sizeof(b));
    b.n_logs = L;
    b.n_ops = T;
    b.log_off = log_off.data();
    b.chg_off = chg_off.data();
    b.op_id = op_id.data();
    b.ref_a = b.ref_b = zero64.data();
    b.payload = pay.data();
    b.action = act.data();
    b.mark_type = b.side_a = b.side_b = zero8.data();
    b.chg_hdr = hdr.data();
    b.chg_env = env.data();
    b.max_actors = na;
    /* three cuts per log */
    std::vector<uint32_t> src, clocks, prefix;
    for (uint32_t k = 0; k < L; ++k)
        for (int v = 0; v < 3; ++v) {
            src.push_back(k);
            const uint32_t n = (uint32_t)logs[k].chg.size();
            prefix.push_back(v == 0 ? 0 : v == 1 ? n + 3 : rnd(n + 1));
            for (uint32_t a = 0; a < na; ++a) clocks.push_back(v == 0 ? 0 : v == 1 ? PTX_VERSION_ALL : rnd(n / logs[k].na + 2));
        }
    const uint32_t P = (uint32_t)src.size();
    for (int reverse = 0; reverse < 3; ++reverse) {
        /* outputs of exactly the worst-case size: the sanitizer sees every store past them */
        size_t cap = 0, ccap = 0;
        for (uint32_t s : src) cap += log_off[s + 1] - log_off[s], ccap += chg_off[s + 1] - chg_off[s];
        std::vector<uint32_t> status(P), n_kept(P), first_row(P), clocks_out((size_t)P * na), o_pay(cap), o_hdr(ccap);
        std::vector<uint64_t> o_log(P + 1), o_chg(P + 1), o_id(cap), o_ra(cap), o_rb(cap);
        std::vector<uint8_t> o_act(cap), o_mt(cap), o_sa(cap), o_sb(cap);
        std::vector<uint16_t> o_env(ccap * es);
        const int rc = ptx_emu_versions(&b, P, src.data(), use_prefix ? nullptr : clocks.data(), use_prefix ? prefix.data() : nullptr, then_rest ? PTX_VERSIONS_THEN_REST : 0u, reverse,
                                        status.data(), n_kept.data(), first_row.data(), clocks_out.data(), o_log.data(), o_chg.data(), o_id.data(), o_ra.data(), o_rb.data(), o_pay.data(),
                                        o_act.data(), o_mt.data(), o_sa.data(), o_sb.data(), o_hdr.data(), o_env.data(), nullptr);
        if (rc != 0) return printf("%s: ptx_emu_versions returned %d\n", what, rc), 1;
        for (uint32_t p = 0; p < P; ++p) {
            const Log& l = logs[src[p]];
            std::vector<uint32_t> clk(clocks.begin() + (size_t)p * na, clocks.begin() + (size_t)(p + 1) * na);
            const Want w = filter(l, clk.data(), use_prefix ? &prefix[p] : nullptr, then_rest);
            if (status[p] != w.status || n_kept[p] != w.n_kept || first_row[p] != w.first_row || o_chg[p + 1] - o_chg[p] != w.order.size())
                return printf("%s: cut %u: status %u kept %u first_row %u changes %llu, expected %u %u %u %zu (lane order %d)\n", what, p, status[p], n_kept[p], first_row[p],
                              (unsigned long long)(o_chg[p + 1] - o_chg[p]), w.status, w.n_kept, w.first_row, w.order.size(), reverse), 1;
            for (uint32_t a = 0; a < na; ++a)
                if (clocks_out[(size_t)p * na + a] != (a < l.na ? w.clock[a] : 0u)) return printf("%s: cut %u: effective clock of actor %u\n", what, p, a), 1;
            uint64_t row = o_log[p];
            for (size_t j = 0; j < w.order.size(); ++j) {
                const uint32_t i = w.order[j];
                const Chg& c = l.chg[i];
                if (o_hdr[o_chg[p] + j] != (c.actor << PTX_CHG_ACTOR_SHIFT | c.nops) || o_env[(o_chg[p] + j) * es] != c.seq) return printf("%s: cut %u: change %zu differs\n", what, p, j), 1;
                for (uint32_t bb = 0; bb < l.na; ++bb)
                    if (o_env[(o_chg[p] + j) * es + 1 + bb] != c.deps[bb]) return printf("%s: cut %u: deps of change %zu differ\n", what, p, j), 1;
                for (uint32_t r = 0; r < c.nops; ++r, ++row)
                    if (o_id[row] != ((((uint64_t)(100000u * src[p] + 8u * i + r + 1u)) << 32) | c.actor) || o_act[row] != PTX_ACT_INSERT || o_pay[row] != 7)
                        return printf("%s: cut %u: row %u of change %zu differs (lane order %d)\n", what, p, r, j, reverse), 1;
            }
            if (row != o_log[p + 1]) return printf("%s: cut %u: %llu rows, expected %llu\n", what, p, (unsigned long long)(o_log[p + 1] - o_log[p]), (unsigned long long)(row - o_log[p])), 1;
        }
    }
    return 0;
}

int main() {
    for (uint32_t na : {1u, 2u, 3u, 4u, 7u, 8u, 15u, 17u}) { /* one batch per actor count: envelope rows of 4 .. 20 u16 */
        std::vector<Log> logs;
        for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 129u, 136u, 300u}) logs.push_back(make_log(na, n));
        for (int then_rest = 0; then_rest < 2; ++then_rest) {
            if (run(logs, false, then_rest != 0, then_rest ? "clock cuts, then the rest" : "clock cuts")) return 1;
            if (run(logs, true, then_rest != 0, then_rest ? "prefix cuts, then the rest" : "prefix cuts")) return 1;
        }
    }
    printf("version emulation ok\n");
    return 0;
}
