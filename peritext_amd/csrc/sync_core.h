/*
 * sync_core.h — the sync between two replicas of a document on the device: which Changes of a source replica a target replica lacks, and
 * the order in which the target ends up applying them.
 *
 * What it replaces, per (source, target) pair — the two calls the reference's multi-replica loop makes after every edit (test/fuzz.ts:181-199) and
 * the editor makes through ChangeQueue / bridge.ts:
 *   getMissingChanges(source, target)   reference/test/merge.ts:25-38   the vector-clock difference
 *   applyChanges(target, missing)       reference/test/merge.ts:4-22    apply the bag, re-queueing whatever throws the causal RangeError
 *
 * A log is what a replica applied, in application order, with its Change envelope (include/peritext_hip.h).  Both logs of a pair are replicas of the
 * SAME document: they share the actor ranks.
 *
 *   Clocks        clock[a] = the largest seq of actor a in the log, 0 = the log holds no change of a (micromerge.ts:511 sets clock[actor] = seq;
 *                 `=== undefined`, merge.ts:30, is the 0).  Exact lo | hi << 16 when the batch carries chg_env_hi.
 *   Missing bag   merge.ts:29 walks Object.entries(source.clock): the actors in the order of their FIRST APPEARANCE in the source log (change() and
 *                 applyChange both create the key at the actor's first change).  Per actor: the source's changes of that actor with seq > the
 *                 target's clock[a], in log order (merge.ts:30-35; an actor the target never saw contributes all of them, :30-32).
 *   Retry order   merge.ts:7-20: take the head, admit it as applyChange does (micromerge.ts:499-511: seq == clock[actor] + 1 and clock[b] >= deps[b]
 *                 for every non-zero dep, the own actor's included), push it to the back on failure.  Failures keep their relative order, so the
 *                 loop is a sequence of PASSES over what is left, actor run by actor run; inside a run the seq check makes every change behind the
 *                 first failure fail too.  The output is the source's change indices in the order they were admitted.
 *   The guard     merge.ts:18 throws once the 10 002nd attempt has been made, also when that attempt emptied the queue.  The attempts T of a pair
 *                 are the sum of the queue lengths at the pass starts; T > max_attempts (non-zero; 10 001 = the reference) is
 *                 PTX_ERR_SYNC_NOT_CONVERGED.  A pass that admits nothing is the same status whatever max_attempts is: the reference spins into
 *                 its guard there (a source log no replica could have applied), the kernel terminates.
 *   Op-level errors  merge.ts:15 catches EVERY error, the op-level ones too.  This code looks at the envelope only: a change whose ops would throw
 *                 is ordered like any other, and the grown log reports its op-level status at its merge.
 * A failed pair contributes nothing (the reference leaves the target half-updated).
 *
 * Two kernels, written against the platform layer like the other cores (hipcc: the product; g++ -DPTX_EMU: tests/emu/emu_sync.cc):
 *   ptx_sync_plan_pair    ONE 64-lane wave per pair.  LDS holds a few words per ACTOR (the running clock, first appearance, actor order, run bounds and
 *                         cursors) and one 64-word chunk buffer; everything proportional to a log — the missing queue, the admitted order, the two
 *                         row-offset scans — is u32 per source change in global scratch.
 *   ptx_sync_gather_pair  one workgroup per pair: the op rows of the admitted changes, one thread per ROW (row -> change by binary search in the
 *                         scanned offsets: changes average 1.3 ops), then chg_hdr and the envelope rows one thread per word.
 */
#pragma once
#include "gen_core.h"

#define PTX_SYNC_NONE 0xFFFFFFFFu

struct PtxSyncArgs {
    /* the base batch (resident) */
    const uint64_t* log_off;
    const uint64_t* chg_off;
    const uint32_t* chg_hdr;
    const uint16_t* chg_env;
    const uint16_t* chg_env_hi; /* NULL: narrow envelope (65 535 = saturated) */
    uint32_t max_actors;
    /* the pairs */
    uint32_t n_pairs;
    uint32_t max_attempts;      /* 0 = unbounded */
    const uint32_t* src_log;    /* [n_pairs] */
    const uint32_t* dst_log;    /* [n_pairs] */
    const uint64_t* scr_off;    /* [n_pairs + 1] in u32 words: the slice of pair p holds 4 * (source changes + 1) words */
    uint32_t* scratch;          /* per pair: queue[n] | order[n] | src_row[n + 1] | dst_row[n + 1] */
    /* plan output, per pair */
    uint32_t* status;           /* PTX_OK / PTX_ERR_SYNC_NOT_CONVERGED / PTX_ERR_CAPACITY / PTX_ERR_BAD_OP (an actor rank >= max_actors) */
    uint32_t* n_admitted;       /* changes of `order` (0 on failure) */
    uint32_t* n_rows;           /* their op rows */
    uint32_t lds_bytes;
};

struct PtxSyncHdr {
    uint32_t bad;       /* PTX_ERR_* found while striding the envelopes */
    uint32_t n_present; /* actors of the source log */
    uint32_t run;       /* cursor of the scans / slots */
    uint32_t pad;
    uint32_t chunk[64]; /* the actor of the chunk's changes | bit 31: missing */
};

PTX_HD uint64_t ptx_sync_lds_need(uint64_t na) { return ptx_a16(sizeof(PtxSyncHdr)) + 6 * ptx_a16(4 * (na + 1)); }
PTX_HD uint64_t ptx_sync_scratch_words(uint64_t n_src_changes) { return 4 * (n_src_changes + 1); }

/* the pair rules of ptx_sync_replicas: 0 = fine, 1 = a pair names a log the batch does not have, 2 = a log is the target of two pairs.  `seen`: [n_logs] bytes of the caller's, zeroed here */
static inline int ptx_sync_check_pairs(uint32_t n_logs, uint32_t n_pairs, const uint32_t* src_log, const uint32_t* dst_log, uint8_t* seen) {
    for (uint32_t l = 0; l < n_logs; ++l) seen[l] = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (src_log[p] >= n_logs || dst_log[p] >= n_logs) return 1;
        if (seen[dst_log[p]]) return 2;
        seen[dst_log[p]] = 1;
    }
    return 0;
}

/* value k of envelope row c (0 = seq, 1 + b = deps[b]) */
PTX_DEV uint32_t ptx_sync_env(const PtxSyncArgs& A, uint32_t es, uint64_t c, uint32_t k) {
    const uint32_t lo = A.chg_env[c * es + k];
    return A.chg_env_hi ? lo | ((uint32_t)A.chg_env_hi[c * es + k] << 16) : lo;
}
/* a narrow row holds a saturated value: its seq / deps cannot be compared */
PTX_DEV bool ptx_sync_row_saturated(const PtxSyncArgs& A, uint32_t es, uint64_t c, uint32_t na) {
    if (A.chg_env_hi) return false;
    bool sat = false;
    for (uint32_t k = 0; k <= na; ++k) sat |= A.chg_env[c * es + k] == PTX_ENV_SATURATED;
    return sat;
}
/* applyChange's admission (micromerge.ts:499-511) of the change that stands `ahead` places behind the actor's clock in its run: the ones before it count as admitted */
PTX_DEV bool ptx_sync_admits(const PtxSyncArgs& A, uint32_t es, uint64_t c, uint32_t a, uint32_t clk_a, uint32_t ahead, const uint32_t* clock, uint32_t na) {
    const uint32_t seq = ptx_sync_env(A, es, c, 0);
    if (seq != clk_a + ahead + 1u) return false;
    for (uint32_t b = 0; b < na; ++b) {
        const uint32_t d = ptx_sync_env(A, es, c, 1u + b);
        if (d != 0u && (b == a ? seq - 1u : clock[b]) < d) return false;
    }
    return true;
}

template <uint32_t kThreads>
PTX_DEV void ptx_sync_plan_pair(const PtxSyncArgs& A, uint32_t pair, uint8_t* lds) {
    PtxSyncHdr* H = (PtxSyncHdr*)lds;
    const uint32_t s = A.src_log[pair], t = A.dst_log[pair], na = A.max_actors, es = PTX_ENV_STRIDE(na);
    const uint64_t s0 = A.chg_off[s], t0 = A.chg_off[t];
    const uint32_t ns = (uint32_t)(A.chg_off[s + 1] - s0), nt = (uint32_t)(A.chg_off[t + 1] - t0);
    uint32_t* queue = A.scratch + A.scr_off[pair];
    uint32_t* order = queue + ns;
    uint32_t* src_row = order + ns;          /* [ns + 1] first op row of source change c, relative to the log */
    uint32_t* dst_row = src_row + ns + 1u;   /* [admitted + 1] first row of the k-th admitted change in `more` */

#define PTX_SYNC_DONE(code_, adm_, rows_)             \
    do {                                              \
        PTX_SYNC();                                   \
        PTX_LEADER {                                  \
            A.status[pair] = (code_);                 \
            A.n_admitted[pair] = (adm_);              \
            A.n_rows[pair] = (rows_);                 \
        }                                             \
        return;                                       \
    } while (0)

    if (s == t || ns == 0u) PTX_SYNC_DONE(PTX_OK, 0u, 0u);
    PtxBump bp;
    bp.base = lds;
    bp.off = (uint32_t)ptx_a16(sizeof(PtxSyncHdr));
    bp.cap = A.lds_bytes;
    bp.high = bp.off;
    bp.overflow = false;
    uint32_t* clock = ptx_alloc<uint32_t>(bp, na + 1); /* the target's clock, advanced by every admission */
    uint32_t* first = ptx_alloc<uint32_t>(bp, na + 1); /* first appearance in the source log */
    uint32_t* ord = ptx_alloc<uint32_t>(bp, na + 1);   /* the actors of the source log by first appearance */
    uint32_t* cnt = ptx_alloc<uint32_t>(bp, na + 1);   /* missing changes per actor */
    uint32_t* cur = ptx_alloc<uint32_t>(bp, na + 1);   /* queue position of the actor's next change */
    uint32_t* end = ptx_alloc<uint32_t>(bp, na + 1);   /* ... of the end of its run */
    if (bp.overflow || (uint64_t)ns * es > 0xFFFFFFFFull) PTX_SYNC_DONE(PTX_ERR_CAPACITY, 0u, 0u); /* (the gather indexes a pair's envelope words with 32 bits) */

    PTX_FOR(a, na + 1) {
        clock[a] = 0;
        first[a] = PTX_SYNC_NONE;
        cnt[a] = 0;
        ord[a] = 0;
    }
    PTX_LEADER {
        H->bad = 0;
        H->n_present = 0;
        H->run = 0;
    }
    PTX_SYNC();
    /* ---- the target's clock; the source's first appearances ---- */
    PTX_FOR(c, nt) {
        const uint32_t a = A.chg_hdr[t0 + c] >> PTX_CHG_ACTOR_SHIFT;
        if (a >= na) ptx_atomic_max(&H->bad, PTX_ERR_BAD_OP);
        else {
            if (ptx_sync_row_saturated(A, es, t0 + c, na)) ptx_atomic_max(&H->bad, PTX_ERR_CAPACITY);
            ptx_atomic_max(&clock[a], ptx_sync_env(A, es, t0 + c, 0));
        }
    }
    PTX_FOR(c, ns) {
        const uint32_t a = A.chg_hdr[s0 + c] >> PTX_CHG_ACTOR_SHIFT;
        if (a >= na) ptx_atomic_max(&H->bad, PTX_ERR_BAD_OP);
        else {
            if (ptx_sync_row_saturated(A, es, s0 + c, na)) ptx_atomic_max(&H->bad, PTX_ERR_CAPACITY);
            ptx_atomic_min(&first[a], c);
        }
    }
    PTX_SYNC();
    if (H->bad) PTX_SYNC_DONE(H->bad == PTX_ERR_BAD_OP ? PTX_ERR_BAD_OP : PTX_ERR_CAPACITY, 0u, 0u); /* (PTX_ERR_CAPACITY < PTX_ERR_BAD_OP: the maximum of the two) */
    /* ---- missing changes per actor; the first op row of every source change (an exclusive scan of nops, 64 changes per step) ---- */
    for (uint32_t base = 0; base < ns; base += 64u) {
        PTX_GEN_FOR(l, 64u) {
            const uint32_t c = base + l;
            uint32_t nops = 0;
            if (c < ns) {
                const uint32_t h = A.chg_hdr[s0 + c], a = h >> PTX_CHG_ACTOR_SHIFT;
                nops = h & PTX_CHG_NOPS;
                if (ptx_sync_env(A, es, s0 + c, 0) > clock[a]) ptx_atomic_add(&cnt[a], 1u);
            }
            const uint32_t at = ptx_append_n(&H->run, nops);
            if (c < ns) src_row[c] = at;
        }
    }
    PTX_SYNC();
    /* ---- the actors in first-appearance order (first[] values are distinct change indices), their runs back to back ---- */
    PTX_FOR(a, na) {
        if (first[a] != PTX_SYNC_NONE) {
            uint32_t pos = 0;
            for (uint32_t b = 0; b < na; ++b) pos += first[b] < first[a] ? 1u : 0u;
            ord[pos] = a;
            ptx_atomic_add(&H->n_present, 1u);
        }
    }
    PTX_SYNC();
    const uint32_t n_present = H->n_present;
    PTX_LEADER {
        src_row[ns] = H->run;
        uint32_t run = 0;
        for (uint32_t k = 0; k < n_present; ++k) {
            const uint32_t a = ord[k];
            cur[a] = run;
            run += cnt[a];
            end[a] = run;
        }
        H->run = run;
    }
    PTX_SYNC();
    const uint32_t n_missing = H->run;
    /* ---- the missing queue: a STABLE multi-way partition of the source's change indices, 64 changes per step; per actor present in the step the slots are
     *      prefix counts over its ballot and ONE bump of the actor's cursor ---- */
    for (uint32_t base = 0; base < ns && n_missing; base += 64u) {
        PTX_GEN_FOR(l, 64u) {
            const uint32_t c = base + l;
            uint32_t w = 0;
            if (c < ns) {
                w = A.chg_hdr[s0 + c] >> PTX_CHG_ACTOR_SHIFT;
                if (ptx_sync_env(A, es, s0 + c, 0) > clock[w]) w |= 0x80000000u;
            }
            H->chunk[l] = w;
        }
        PTX_SYNC();
        PTX_BALLOT64(todo0, l0, (H->chunk[l0] >> 31) != 0u)
        uint64_t todo = todo0;
        while (todo) {
            const uint32_t a = H->chunk[ptx_ffs64(todo)] & 0x7FFFFFFFu;
            PTX_BALLOT64(same, l1, ((todo >> l1) & 1ull) && (H->chunk[l1] & 0x7FFFFFFFu) == a)
            const uint32_t at = cur[a];
            PTX_GEN_FOR(l, 64u) {
                if ((same >> l) & 1ull) queue[at + (uint32_t)__builtin_popcountll(same & ((1ull << l) - 1ull))] = base + l;
            }
            PTX_SYNC();
            PTX_LEADER { cur[a] = at + (uint32_t)__builtin_popcountll(same); }
            PTX_SYNC();
            todo &= ~same;
        }
    }
    PTX_SYNC();
    PTX_FOR(a, na) {
        if (first[a] != PTX_SYNC_NONE) cur[a] = end[a] - cnt[a]; /* back to the start of the run */
    }
    PTX_SYNC();
    /* ---- the passes of merge.ts:7-20 ---- */
    uint32_t n_adm = 0;
    uint64_t attempts = 0;
    while (n_adm < n_missing) {
        attempts += (uint64_t)(n_missing - n_adm); /* every change still queued is attempted once per pass */
        if (A.max_attempts && attempts > (uint64_t)A.max_attempts) PTX_SYNC_DONE(PTX_ERR_SYNC_NOT_CONVERGED, 0u, 0u);
        const uint32_t before = n_adm;
        for (uint32_t k = 0; k < n_present; ++k) {
            const uint32_t a = ord[k];
            uint32_t at = cur[a], clk_a = clock[a];
            const uint32_t stop = end[a];
            while (at < stop) {
                const uint32_t m = stop - at < 64u ? stop - at : 64u;
                PTX_BALLOT64(fails, l, l < m && !ptx_sync_admits(A, es, s0 + queue[at + l], a, clk_a, l, clock, na))
                const uint32_t ok = fails ? ptx_ffs64(fails) : m; /* the admitted prefix */
                PTX_GEN_FOR(l, ok) order[n_adm + l] = queue[at + l];
                at += ok;
                clk_a += ok;
                n_adm += ok;
                if (ok) { /* the next chunk, and the other actors' deps, see the advanced clock */
                    PTX_SYNC();
                    PTX_LEADER {
                        clock[a] = clk_a;
                        cur[a] = at;
                    }
                    PTX_SYNC();
                }
                if (ok < m) break; /* a failure ends the actor's run for this pass: the changes behind it fail the seq check */
            }
        }
        if (n_adm == before) PTX_SYNC_DONE(PTX_ERR_SYNC_NOT_CONVERGED, 0u, 0u); /* nobody can apply this log */
    }
    PTX_SYNC();
    /* ---- first row of every admitted change in `more` ---- */
    PTX_LEADER { H->run = 0; }
    PTX_SYNC();
    for (uint32_t base = 0; base < n_adm; base += 64u) {
        PTX_GEN_FOR(l, 64u) {
            const uint32_t k = base + l;
            const uint32_t nops = k < n_adm ? A.chg_hdr[s0 + order[k]] & PTX_CHG_NOPS : 0u;
            const uint32_t at = ptx_append_n(&H->run, nops);
            if (k < n_adm) dst_row[k] = at;
        }
    }
    PTX_SYNC();
    const uint32_t rows = H->run;
    PTX_LEADER { dst_row[n_adm] = rows; }
    PTX_SYNC_DONE(PTX_OK, n_adm, rows);
#undef PTX_SYNC_DONE
}

/* destination of the gather: the columns of `more`, its offsets */
struct PtxSyncGatherArgs {
    const uint64_t *op_id, *ref_a, *ref_b;
    const uint32_t* payload;
    const uint8_t *action, *mark_type, *side_a, *side_b;
    uint64_t *o_op_id, *o_ref_a, *o_ref_b;
    uint32_t* o_payload;
    uint8_t *o_action, *o_mark_type, *o_side_a, *o_side_b;
    uint32_t* o_chg_hdr;
    uint16_t* o_chg_env;
    uint16_t* o_chg_env_hi;     /* NULL iff the base has no wide column */
    const uint64_t* o_log_off;  /* [n_logs + 1] of `more` */
    const uint64_t* o_chg_off;
};

template <uint32_t kThreads>
PTX_DEV void ptx_sync_gather_pair(const PtxSyncArgs& A, const PtxSyncGatherArgs& G, uint32_t pair) {
    const uint32_t n_adm = A.n_admitted[pair];
    if (n_adm == 0u) return;
    const uint32_t s = A.src_log[pair], t = A.dst_log[pair], es = PTX_ENV_STRIDE(A.max_actors);
    const uint64_t s0 = A.chg_off[s], r0 = A.log_off[s], d0 = G.o_log_off[t], dc0 = G.o_chg_off[t];
    const uint32_t ns = (uint32_t)(A.chg_off[s + 1] - s0);
    const uint32_t* order = A.scratch + A.scr_off[pair] + ns;
    const uint32_t* src_row = order + ns;
    const uint32_t* dst_row = src_row + ns + 1u;
    const uint32_t rows = dst_row[n_adm];
    PTX_FOR(r, rows) {
        uint32_t lo = 0, hi = n_adm; /* the last k with dst_row[k] <= r (changes without ops share their successor's first row) */
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (dst_row[mid] <= r) lo = mid;
            else hi = mid;
        }
        const uint64_t from = r0 + src_row[order[lo]] + (r - dst_row[lo]), to = d0 + r;
        G.o_op_id[to] = G.op_id[from];
        G.o_ref_a[to] = G.ref_a[from];
        G.o_ref_b[to] = G.ref_b[from];
        G.o_payload[to] = G.payload[from];
        G.o_action[to] = G.action[from];
        G.o_mark_type[to] = G.mark_type[from];
        G.o_side_a[to] = G.side_a[from];
        G.o_side_b[to] = G.side_b[from];
    }
    PTX_FOR(k, n_adm) G.o_chg_hdr[dc0 + k] = A.chg_hdr[s0 + order[k]];
    /* envelope rows are 8-byte aligned multiples of four u16: one thread per 32-bit word */
    const uint32_t ew = es >> 1;
    PTX_FOR(i, n_adm * ew) {
        const uint32_t k = i / ew, w = i - k * ew;
        ((uint32_t*)(G.o_chg_env + (dc0 + k) * es))[w] = ((const uint32_t*)(A.chg_env + (s0 + order[k]) * es))[w];
        if (G.o_chg_env_hi) ((uint32_t*)(G.o_chg_env_hi + (dc0 + k) * es))[w] = ((const uint32_t*)(A.chg_env_hi + (s0 + order[k]) * es))[w];
    }
}
