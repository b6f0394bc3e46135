/*
 * Stand-alone sanitizer program of the sync emulation — TEST TOOLING ONLY (tests/test_emu_sync.py compiles it with g++ -fsanitize=address,undefined and runs
 * it as a child process).  It builds the chunk-edge and ping-pong envelopes itself (one-op changes), runs plan + gather of sync_core.h through emu_sync.cc in the
 * three lane orders and checks the admitted order against the sequential queue of reference/test/merge.ts:4-22 restated below.
 */
#include "emu_sync.cc"

#include <stdio.h>

#include <deque>
#include <vector>

struct Chg {
    uint32_t actor, seq;
    std::vector<uint32_t> deps; /* [na] */
};
struct Doc {
    uint32_t na;
    std::vector<Chg> src, dst;
};

/* getMissingChanges + applyChanges, one change at a time: the admitted source indices, or `false` once more than max_attempts attempts were made / nothing moves */
static bool queue_sync(const Doc& d, uint32_t max_attempts, std::vector<uint32_t>& order) {
    std::vector<uint32_t> clock(d.na, 0), seen;
    for (const Chg& c : d.dst) clock[c.actor] = c.seq > clock[c.actor] ? c.seq : clock[c.actor];
    std::deque<uint32_t> q;
    for (const Chg& c : d.src) {
        bool known = false;
        for (uint32_t a : seen) known |= a == c.actor;
        if (!known) seen.push_back(c.actor);
    }
    for (uint32_t a : seen)
        for (uint32_t i = 0; i < d.src.size(); ++i)
            if (d.src[i].actor == a && d.src[i].seq > clock[a]) q.push_back(i);
    uint64_t attempts = 0, failed_in_a_row = 0;
    while (!q.empty()) {
        const uint32_t i = q.front();
        q.pop_front();
        const Chg& c = d.src[i];
        bool ok = c.seq == clock[c.actor] + 1;
        for (uint32_t b = 0; ok && b < d.na; ++b) ok = c.deps[b] == 0 || clock[b] >= c.deps[b];
        if (ok) clock[c.actor] = c.seq, order.push_back(i), failed_in_a_row = 0;
        else q.push_back(i), ++failed_in_a_row;
        if (++attempts > max_attempts && max_attempts) return false;
        if (failed_in_a_row && failed_in_a_row >= q.size()) return false;
    }
    return true;
}

static int run(const std::vector<Doc>& docs, uint32_t max_attempts, const char* what) {
    /* one batch: document k = logs 2k (source), 2k + 1 (target); every change is one op whose id says where it came from */
    uint32_t na = 1;
    for (const Doc& d : docs) na = d.na > na ? d.na : na;
    const uint32_t es = PTX_ENV_STRIDE(na), L = 2 * (uint32_t)docs.size();
    std::vector<uint64_t> off(1, 0), op_id, zero64;
    std::vector<uint32_t> hdr, src_log, dst_log;
    std::vector<uint16_t> env;
    for (uint32_t k = 0; k < docs.size(); ++k) {
        for (int side = 0; side < 2; ++side) {
            const std::vector<Chg>& log = side ? docs[k].dst : docs[k].src;
            for (uint32_t i = 0; i < log.size(); ++i) {
                hdr.push_back(log[i].actor << PTX_CHG_ACTOR_SHIFT | 1u);
                std::vector<uint16_t> row(es, 0);
                row[0] = (uint16_t)log[i].seq;
                for (uint32_t b = 0; b < docs[k].na; ++b) row[1 + b] = (uint16_t)log[i].deps[b];
                env.insert(env.end(), row.begin(), row.end());
                op_id.push_back(((uint64_t)(1000u * k + i + 1u) << 32) | log[i].actor);
            }
            off.push_back(op_id.size());
        }
        src_log.push_back(2 * k);
        dst_log.push_back(2 * k + 1);
    }
    const size_t T = op_id.size();
    zero64.assign(T + 1, 0);
    std::vector<uint32_t> pay(T + 1, 7);
    std::vector<uint8_t> act(T + 1, PTX_ACT_INSERT), zero8(T + 1, 0);
    ptx_batch b;
    memset(&b, 0, sizeof(b));
    b.n_logs = L;
    b.n_ops = T;
    b.log_off = b.chg_off = off.data(); /* one op per change: the same offsets */
    b.op_id = op_id.data();
    b.ref_a = b.ref_b = zero64.data();
    b.payload = pay.data();
    b.action = act.data();
    b.mark_type = b.side_a = b.side_b = zero8.data();
    b.chg_hdr = hdr.data();
    b.chg_env = env.data();
    b.max_actors = na;
    for (int reverse = 0; reverse < 3; ++reverse) {
        const uint32_t P = (uint32_t)docs.size();
        /* outputs of exactly the worst-case size: the sanitizer sees every store past them */
        size_t cap = 0;
        for (const Doc& d : docs) cap += d.src.size();
        std::vector<uint32_t> status(P), n_adm(P), n_rows(P), o_pay(cap), o_hdr(cap);
        std::vector<uint64_t> o_log(L + 1), o_chg(L + 1), o_id(cap), o_ra(cap), o_rb(cap);
        std::vector<uint8_t> o_act(cap), o_mt(cap), o_sa(cap), o_sb(cap);
        std::vector<uint16_t> o_env(cap * es);
        const int rc = ptx_emu_sync(&b, P, src_log.data(), dst_log.data(), max_attempts, reverse, status.data(), n_adm.data(), n_rows.data(), o_log.data(), o_chg.data(), o_id.data(),
                                    o_ra.data(), o_rb.data(), o_pay.data(), o_act.data(), o_mt.data(), o_sa.data(), o_sb.data(), o_hdr.data(), o_env.data(), nullptr);
        if (rc != 0) return printf("%s: ptx_emu_sync returned %d\n", what, rc), 1;
        for (uint32_t k = 0; k < P; ++k) {
            std::vector<uint32_t> want;
            const bool ok = queue_sync(docs[k], max_attempts, want);
            if ((status[k] == PTX_OK) != ok || (!ok && status[k] != PTX_ERR_SYNC_NOT_CONVERGED)) return printf("%s: document %u status %u, the queue %s\n", what, k, status[k], ok ? "converged" : "did not"), 1;
            const uint64_t at = o_chg[2 * k + 1], n = o_chg[2 * k + 2] - at;
            if (n != (ok ? want.size() : 0) || n != n_adm[k] || o_log[2 * k + 2] - o_log[2 * k + 1] != n) return printf("%s: document %u admits %llu changes, expected %zu\n", what, k, (unsigned long long)n, want.size()), 1;
            for (uint64_t j = 0; j < n; ++j) {
                const Chg& c = docs[k].src[want[j]];
                if (o_id[o_log[2 * k + 1] + j] != op_id[off[2 * k] + want[j]] || o_hdr[at + j] != (c.actor << PTX_CHG_ACTOR_SHIFT | 1u) || o_env[(at + j) * es] != c.seq || o_act[o_log[2 * k + 1] + j] != PTX_ACT_INSERT ||
                    o_pay[o_log[2 * k + 1] + j] != 7)
                    return printf("%s: document %u, admitted change %llu differs (lane order %d)\n", what, k, (unsigned long long)j, reverse), 1;
                for (uint32_t bb = 0; bb < docs[k].na; ++bb)
                    if (o_env[(at + j) * es + 1 + bb] != c.deps[bb]) return printf("%s: document %u, deps of admitted change %llu differ\n", what, k, (unsigned long long)j), 1;
            }
        }
    }
    return 0;
}

static Chg chg(uint32_t na, uint32_t actor, uint32_t seq) { return Chg{actor, seq, std::vector<uint32_t>(na, 0)}; }

int main() {
    std::vector<Doc> edges;
    for (uint32_t n : {63u, 64u, 65u, 129u}) { /* one actor's run across the 64-change steps */
        Doc d{2, {chg(2, 0, 1)}, {chg(2, 0, 1)}};
        for (uint32_t k = 0; k < n; ++k) d.src.push_back(chg(2, 1, k + 1)), d.src.back().deps[0] = 1;
        edges.push_back(d);
    }
    for (uint32_t f : {0u, 63u, 64u}) { /* the first failing change at lane 0, lane 63, the first lane of the second chunk */
        Doc d{3, {chg(3, 0, 1)}, {chg(3, 0, 1)}};
        for (uint32_t k = 0; k < 5; ++k) d.src.push_back(chg(3, 1, k + 1)), d.dst.push_back(chg(3, 1, k + 1));
        d.src.push_back(chg(3, 2, 1));
        for (uint32_t k = 0; k < 135; ++k) {
            d.src.push_back(chg(3, 1, k + 6));
            if (k == f) d.src.back().deps[2] = 1;
        }
        edges.push_back(d);
    }
    { /* deps that are not monotone along a run, an actor nobody can admit, an empty source */
        Doc d{3, {chg(3, 0, 1), chg(3, 1, 1), chg(3, 2, 1), chg(3, 2, 2), chg(3, 1, 2), chg(3, 1, 3), chg(3, 1, 4)}, {chg(3, 0, 1), chg(3, 2, 1)}};
        d.src[4].deps[2] = 2;
        d.src[5].deps[2] = 1;
        edges.push_back(d);
        Doc stuck{2, {chg(2, 0, 1), chg(2, 1, 1), chg(2, 1, 2)}, {chg(2, 0, 1)}};
        stuck.src[1].deps[0] = 7;
        edges.push_back(stuck);
        edges.push_back(Doc{2, {}, {chg(2, 0, 1)}});
    }
    if (run(edges, 10001, "chunk edges")) return 1;
    std::vector<Doc> pp;
    const uint32_t shapes[4][2] = {{99, 0}, {100, 0}, {99, 101}, {99, 102}}; /* rounds, independent changes: T = 9 900, 10 100, 10 001, 10 002 */
    for (const auto& s : shapes) {
        Doc d{3, {}, {}};
        for (uint32_t k = 1; k <= s[0]; ++k) {
            d.src.push_back(chg(3, 0, k));
            d.src.back().deps[1] = k - 1;
            d.src.push_back(chg(3, 1, k));
            d.src.back().deps[0] = k;
        }
        for (uint32_t k = 1; k <= s[1]; ++k) d.src.push_back(chg(3, 2, k));
        pp.push_back(d);
    }
    if (run(pp, 10001, "ping-pong, the reference's guard")) return 1;
    if (run(pp, 0, "ping-pong, unbounded")) return 1;
    printf("sync emulation ok\n");
    return 0;
}
