/*
 * version_core.h — a replica log at a past version: which Changes of a resident log make up version V, and (PTX_VERSIONS_THEN_REST) the others behind them.
 *
 * A log is what a replica applied, in application order, with its Change envelope (include/peritext_hip.h).  Cut c reads the source log s = src_log[c];
 * the actor ranks are the batch's own, as for the sync (sync_core.h).
 *
 *   Clock cut     clock[c][a], a u32 per actor rank, max_actors of them.  A change of actor a is KEPT iff seq <= clock[c][a]: micromerge.ts:511 sets
 *                 clock[actor] = seq at every admission, so a replica whose clock says clock[a] holds exactly a's changes 1 .. clock[a].  0 keeps none of
 *                 the actor (`=== undefined`, merge.ts:30), PTX_VERSION_ALL all of them.  Exact lo | hi << 16 where the batch has chg_env_hi.
 *   Prefix cut    prefix[c] = k keeps the first min(k, n) changes: the version the replica itself was at after its k-th applyChange / change().
 *   Kept changes  keep their log order, with their op rows, chg_hdr and envelope rows.  For a causally closed clock (one some replica really had) every dep
 *                 of a kept change stands before it in the source and is itself kept, and each actor's kept changes are a prefix of the actor's run: the cut
 *                 log passes applyChange's admission (micromerge.ts:499-511) in that order.
 *   Closedness    checked here, on the envelope alone: a kept change with a non-zero deps[b], b not its own actor, and deps[b] > clock[c][b] makes the cut
 *                 PTX_ERR_MISSING_DEP — applyChange throws "Missing dependency" (micromerge.ts:505-508) at exactly that change when the kept list is applied
 *                 to a fresh Micromerge.  A prefix cut needs no such check.  The source log is NOT re-admitted: an inadmissible source shows at the cut
 *                 log's merge, as a grown log does after a sync.
 *   Other statuses as for the sync: PTX_ERR_CAPACITY for a narrow envelope with a saturated value (65 535) anywhere in the source log, PTX_ERR_BAD_OP for an
 *                 actor rank >= max_actors.  BAD_OP wins over CAPACITY, CAPACITY over MISSING_DEP.  A failed cut contributes an EMPTY log and zero outputs.
 *   THEN_REST     the cut's log = the kept changes followed by the dropped ones, both in log order (a stable partition instead of a compaction).  Admissible
 *                 too: a dropped change's deps are kept, or dropped and earlier in the log; each actor's run is a kept prefix followed by a dropped suffix.
 *                 first_row[c] = the op rows of the kept part: replayed from there, the patch stream is the Patch[] that takes version V to the present.
 *   Outputs       n_kept[c], first_row[c], clocks_out[c][a] = the largest kept seq of actor a (0 = none): the effective clock of the version.
 *
 * One kernel, written against the platform layer like the other cores (hipcc: the product; g++ -DPTX_EMU: tests/emu/emu_versions.cc):
 *   ptx_version_plan_cut  ONE 64-lane wave per cut.  LDS holds two words per ACTOR (the requested clock, the effective clock) and a header with one 64-word
 *                         chunk buffer; everything proportional to a log is u32 per source change in global scratch, laid out exactly as ptx_sync_plan_pair
 *                         lays it out (queue | order | src_row | dst_row; `queue` holds the dropped run until n_kept is known), so that
 *                         ptx_sync_gather_pair does the copy unchanged with dst_log[c] = c, n_admitted = the changes of the output log, n_rows = their rows.
 */
#pragma once
#include "sync_core.h"

#define PTX_VERSION_KEEP 1u  /* chunk word: the change is kept */
#define PTX_VERSION_VALID 2u /* ... stands inside the log */

struct PtxVersionArgs {
    PtxSyncArgs S;            /* the base batch; n_pairs = the cuts, src_log, dst_log[c] = c, scr_off / scratch, status / n_admitted / n_rows per cut */
    const uint32_t* clocks;   /* [n_cuts * max_actors], or NULL: prefix cuts */
    const uint32_t* prefix;   /* [n_cuts], or NULL: clock cuts */
    uint32_t flags;           /* PTX_VERSIONS_THEN_REST */
    uint32_t* n_kept;         /* [n_cuts] */
    uint32_t* first_row;      /* [n_cuts] op rows of the kept changes */
    uint32_t* clocks_out;     /* [n_cuts * max_actors] */
};

struct PtxVersionHdr {
    uint32_t bad;       /* the largest PTX_ERR_* found */
    uint32_t run;       /* cursor of the row scans */
    uint32_t first_row; /* first row of the first dropped change in the output log */
    uint32_t pad;
    uint32_t chunk[64]; /* PTX_VERSION_KEEP | PTX_VERSION_VALID of the chunk's changes */
};

PTX_HD uint64_t ptx_version_lds_need(uint64_t na) { return ptx_a16(sizeof(PtxVersionHdr)) + 2 * ptx_a16(4 * (na + 1)); }

template <uint32_t kThreads>
PTX_DEV void ptx_version_plan_cut(const PtxVersionArgs& V, uint32_t cut, uint8_t* lds) {
    const PtxSyncArgs& A = V.S;
    PtxVersionHdr* H = (PtxVersionHdr*)lds;
    const uint32_t s = A.src_log[cut], na = A.max_actors, es = PTX_ENV_STRIDE(na);
    const uint64_t s0 = A.chg_off[s];
    const uint32_t ns = (uint32_t)(A.chg_off[s + 1] - s0);
    const bool then_rest = (V.flags & PTX_VERSIONS_THEN_REST) != 0u;
    uint32_t* dropped = A.scratch + A.scr_off[cut]; /* the sync's `queue` slice */
    uint32_t* order = dropped + ns;
    uint32_t* src_row = order + ns;        /* [ns + 1] first op row of source change c, relative to the log */
    uint32_t* dst_row = src_row + ns + 1u; /* [changes of the output log + 1] first row of its k-th change */
    uint32_t* want = (uint32_t*)(lds + ptx_a16(sizeof(PtxVersionHdr))); /* the requested clock */
    uint32_t* eff = want + ptx_a16(4 * (na + 1)) / 4;                   /* the effective clock: the largest kept seq per actor */

#define PTX_VERSION_DONE(code_, out_, rows_, kept_, first_)                                                  \
    do {                                                                                                     \
        PTX_SYNC();                                                                                          \
        const bool ok_ = (code_) == PTX_OK;                                                                  \
        PTX_FOR(a, na) V.clocks_out[(uint64_t)cut * na + a] = ok_ ? eff[a] : 0u;                             \
        PTX_LEADER {                                                                                         \
            A.status[cut] = (code_);                                                                         \
            A.n_admitted[cut] = (out_);                                                                      \
            A.n_rows[cut] = (rows_);                                                                         \
            V.n_kept[cut] = (kept_);                                                                         \
            V.first_row[cut] = (first_);                                                                     \
        }                                                                                                    \
        return;                                                                                              \
    } while (0)

    if (ptx_version_lds_need(na) > A.lds_bytes || (uint64_t)ns * es > 0xFFFFFFFFull) PTX_VERSION_DONE(PTX_ERR_CAPACITY, 0u, 0u, 0u, 0u); /* (the gather indexes a cut's envelope words with 32 bits) */
    /* ---- the clock row ---- */
    PTX_FOR(a, na) {
        want[a] = V.clocks ? V.clocks[(uint64_t)cut * na + a] : PTX_VERSION_ALL;
        eff[a] = 0;
    }
    PTX_LEADER {
        H->bad = 0;
        H->run = 0;
        H->first_row = 0;
    }
    PTX_SYNC();
    const uint32_t k_prefix = V.prefix ? V.prefix[cut] : 0u;
    /* ---- keep or drop, 64 changes per step: slots by ballot, the first op row of every source change (an exclusive scan of nops) ---- */
    uint32_t n_kept = 0, n_drop = 0;
    for (uint32_t base = 0; base < ns; base += 64u) {
        PTX_GEN_FOR(l, 64u) {
            const uint32_t c = base + l;
            uint32_t nops = 0, w = 0;
            if (c < ns) {
                const uint32_t h = A.chg_hdr[s0 + c], a = h >> PTX_CHG_ACTOR_SHIFT;
                nops = h & PTX_CHG_NOPS;
                w = PTX_VERSION_VALID;
                if (a >= na) ptx_atomic_max(&H->bad, PTX_ERR_BAD_OP);
                else {
                    if (ptx_sync_row_saturated(A, es, s0 + c, na)) ptx_atomic_max(&H->bad, PTX_ERR_CAPACITY);
                    const uint32_t seq = ptx_sync_env(A, es, s0 + c, 0);
                    if (V.prefix ? c < k_prefix : seq <= want[a]) {
                        w |= PTX_VERSION_KEEP;
                        ptx_atomic_max(&eff[a], seq);
                        if (!V.prefix) { /* closedness: a dep on another actor beyond the requested clock */
                            bool open = false;
                            for (uint32_t b = 0; b < na; ++b) {
                                const uint32_t d = ptx_sync_env(A, es, s0 + c, 1u + b);
                                open |= b != a && d != 0u && d > want[b];
                            }
                            if (open) ptx_atomic_max(&H->bad, PTX_ERR_MISSING_DEP);
                        }
                    }
                }
            }
            H->chunk[l] = w;
            const uint32_t at = ptx_append_n(&H->run, nops + 1u) - c; /* (one more per lane, taken off again: for a step whose counts are ALL zero — 64 changes without ops — ptx_append_n answers 0, not the cursor) */
            if (c < ns) src_row[c] = at;
        }
        PTX_SYNC();
        PTX_BALLOT64(kept, l0, (H->chunk[l0] & PTX_VERSION_KEEP) != 0u)
        PTX_BALLOT64(drop, l1, H->chunk[l1] == PTX_VERSION_VALID)
        PTX_GEN_FOR(l, 64u) {
            const uint64_t below = (1ull << l) - 1ull;
            if ((kept >> l) & 1ull) order[n_kept + (uint32_t)__builtin_popcountll(kept & below)] = base + l;
            else if (then_rest && ((drop >> l) & 1ull)) dropped[n_drop + (uint32_t)__builtin_popcountll(drop & below)] = base + l;
        }
        n_kept += (uint32_t)__builtin_popcountll(kept);
        n_drop += (uint32_t)__builtin_popcountll(drop);
        PTX_SYNC(); /* the chunk buffer is rewritten by the next step */
    }
    PTX_SYNC();
    if (H->bad) PTX_VERSION_DONE(H->bad, 0u, 0u, 0u, 0u);
    PTX_LEADER { src_row[ns] = H->run - ((ns + 63u) & ~63u); }
    /* ---- THEN_REST: the dropped run behind the kept one ---- */
    const uint32_t n_out = then_rest ? ns : n_kept;
    if (then_rest) {
        PTX_FOR(k, n_drop) order[n_kept + k] = dropped[k];
    }
    PTX_SYNC();
    /* ---- first row of every change of the output log ---- */
    PTX_LEADER { H->run = 0; }
    PTX_SYNC();
    for (uint32_t base = 0; base < n_out; base += 64u) {
        PTX_GEN_FOR(l, 64u) {
            const uint32_t k = base + l;
            const uint32_t nops = k < n_out ? A.chg_hdr[s0 + order[k]] & PTX_CHG_NOPS : 0u;
            const uint32_t at = ptx_append_n(&H->run, nops + 1u) - k;
            if (k < n_out) dst_row[k] = at;
            if (k == n_kept) H->first_row = at;
        }
    }
    PTX_SYNC();
    const uint32_t rows = H->run - ((n_out + 63u) & ~63u);
    PTX_LEADER { dst_row[n_out] = rows; }
    PTX_VERSION_DONE(PTX_OK, n_out, rows, n_kept, n_kept < n_out ? H->first_row : rows);
#undef PTX_VERSION_DONE
}
