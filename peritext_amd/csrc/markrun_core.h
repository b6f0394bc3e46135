/*
 * markrun_core.h — queries by FORMAT on a resident text view (view_core.h): the runs of a mark as ranges of visible ELEMENT indexes, chosen on the device
 * (ptx_view_mark_runs), cut by the slice passes without coming down in between (ptx_view_mark_snippets), and the hits of a find filtered by them
 * (ptx_view_find_in_marks).
 *
 * The reference's caller walks the spans getTextWithFormatting returned (reference/src/peritext.ts:337-395) and joins neighbours that carry the mark it asks
 * about: two adjacent spans can both be strong and differ only in em, so a run is a maximal sequence of span rows, not a row.  A selector is (mark_type, id):
 *
 *   strong / em   a row matches iff its attr has the flag; a run is a maximal sequence of consecutive matching rows, run_id 0
 *   link          ... iff PTX_ATTR_LINK is set and (id == PTX_MARK_ANY_ID or the url id equals id); a run also ends where the url id changes; run_id = url id
 *   comment       the runs are the log's cinterval rows whose id matches, in the result's own order (id, start): nothing is joined; run_id = the comment id.  A
 *                 span with PTX_ATTR_COMMENT and no covering interval (`comment: []`) has no row there and so belongs to no run
 *
 * ONE 64-lane wave per log for the reason text_core.h gives, 64 rows per step:
 *
 *   ptx_markrun_walk      row i is a run START iff it matches and row i - 1 does not continue into it (no match, or another url), a run END iff it matches and
 *                         does not continue into row i + 1.  Both neighbours are read from the rows themselves — the line is in the L1 from the lane next door —,
 *                         so a step carries nothing over its edge but two counts.  A ballot each; a start's ordinal is the starts before the step + the popcount
 *                         of the ballot bits below its lane, an end's likewise: starts and ends alternate, so the k-th end closes the k-th start, however many
 *                         steps later.  The end element is the next row's start, n_visible (from the view's own prefix) behind the last row.  The count pass
 *                         returns the starts; the emit pass writes the first `nl` starts and ends and stops once the nl-th END is out.
 *   (the host library scans min(n_runs, cap) into run_off with ptx_text_offsets_kernel)
 *   ptx_markrun_finish_one   a lane per listed run: run_unit = pre[run_start], run_len = pre[run_end] - pre[run_start] and — for snippets — the window
 *                         [run_start - before, run_end + after) saturating like ptx_view_windows_one, with match_unit = pre[run_start] - pre[elem_start]
 *   ptx_markrun_filter_log   one wave per log over the log's UNCAPPED hits (view_core.h's positions and locate passes), 64 per step: a lane binary-searches the
 *                         log's uncapped run list for the last run with start <= hit_start; the hit is kept iff hit_end <= that run's end.  The runs of strong,
 *                         em, link and of ONE comment id are disjoint and ascend by start.  Count, the scan (ptx_find_offsets_kernel applies the cap), then the
 *                         same walk again: a kept hit's slot is the kept before the step + the popcount below its lane — a STABLE compaction of the first
 *                         max_hits_per_log kept hits.
 *
 * Plain vector loads and stores only; written against the platform layer like the other cores: hipcc builds it into the product, tests/emu/emu_markruns.cc plays
 * it on one host thread.
 */
#pragma once
#include "view_core.h"

struct PtxMarkRunArgs {
    const uint64_t* log_off;        /* the view's [n_logs + 1]: where a log's span and cinterval rows start in the merge's result */
    const ptx_span* spans;          /* the result's */
    const ptx_cinterval* cints;     /* ... (PTX_MARK_COMMENT only) */
    const ptx_log_result* logs;     /* ... its per-log rows: n_cintervals of log first_log + l (PTX_MARK_COMMENT only) */
    const uint32_t* status;         /* the view's [n_logs] */
    const uint64_t* span_off;       /* the view's [n_logs + 1] */
    const uint64_t* pre_off;        /* the view's [n_logs + 1] */
    const uint32_t* pre;
    uint32_t first_log, n_logs;
    uint32_t mark_type, id;
    uint32_t cap, n_listed;         /* max_runs_per_log; run_off[n_logs] (finish pass) */
    uint32_t before, after;
    uint32_t* n_runs;               /* [n_logs] ALL runs of the log */
    uint64_t* run_off;              /* [2][n_logs + 1]: row 0 = min(n_runs, cap) from the count pass, scanned by the host's launch; row 1 is not used */
    uint32_t* run_start;            /* [run_off[n_logs]] */
    uint32_t* run_end;
    uint32_t* run_id;
    uint32_t* run_unit;
    uint32_t* run_len;
    uint32_t* win_start;            /* [run_off[n_logs]] or NULL: the slice passes' slice_start */
    uint32_t* win_end;
    uint32_t* match_unit;
};

/* the hit filter's: the uncapped hits and runs in scratch, the kept hits out */
struct PtxMarkFilterArgs {
    uint32_t n_logs, cap;           /* max_hits_per_log */
    const uint64_t* hit_off;        /* [n_logs + 1] of the uncapped hits */
    const uint32_t* hit_unit;
    const uint32_t* hit_start;
    const uint32_t* hit_end;
    const uint64_t* run_off;        /* [n_logs + 1] of the uncapped runs */
    const uint32_t* run_start;
    const uint32_t* run_end;
    uint32_t* n_kept;               /* [n_logs] */
    const uint64_t* out_off;        /* [n_logs + 1] listed kept hits (emit) */
    uint32_t* out_unit;
    uint32_t* out_start;
    uint32_t* out_end;
};

PTX_DEV bool ptx_markrun_match(uint32_t mark_type, uint32_t id, uint32_t attr) {
    if (mark_type == PTX_MARK_STRONG) return (attr & PTX_ATTR_STRONG) != 0u;
    if (mark_type == PTX_MARK_EM) return (attr & PTX_ATTR_EM) != 0u;
    return (attr & PTX_ATTR_LINK) != 0u && (id == PTX_MARK_ANY_ID || (attr & PTX_ATTR_ID_MASK) == id);
}
/* row `a` continues into its successor `b`: both match and, for links, lead to the same url */
PTX_DEV bool ptx_markrun_joined(uint32_t mark_type, uint32_t id, uint32_t a, uint32_t b) {
    return ptx_markrun_match(mark_type, id, a) && ptx_markrun_match(mark_type, id, b) && (mark_type != PTX_MARK_LINK || ((a ^ b) & PTX_ATTR_ID_MASK) == 0u);
}
PTX_DEV bool ptx_markrun_is_start(const PtxMarkRunArgs& A, const ptx_span* sp, uint32_t i) {
    const uint32_t at = sp[i].attr;
    return ptx_markrun_match(A.mark_type, A.id, at) && !(i != 0u && ptx_markrun_joined(A.mark_type, A.id, sp[i - 1u].attr, at));
}
PTX_DEV bool ptx_markrun_is_end(const PtxMarkRunArgs& A, const ptx_span* sp, uint32_t n, uint32_t i) {
    const uint32_t at = sp[i].attr;
    return ptx_markrun_match(A.mark_type, A.id, at) && !(i + 1u < n && ptx_markrun_joined(A.mark_type, A.id, at, sp[i + 1u].attr));
}

/* visible elements of log l: from the view's own prefix, as ptx_slice_visible does for a view */
PTX_DEV uint32_t ptx_markrun_visible(const PtxMarkRunArgs& A, uint32_t l) {
    const uint64_t words = A.pre_off[l + 1u] - A.pre_off[l];
    return words ? (uint32_t)words - 1u : 0u;
}

/* The walk of both passes over log l: the number of its runs — kEmit: of those up to the step in which the nl-th was closed, the first nl written to rs / re / ri. */
template <uint32_t kThreads, bool kEmit>
PTX_DEV uint32_t ptx_markrun_walk(const PtxMarkRunArgs& A, uint32_t l, uint32_t nl, uint32_t* rs, uint32_t* re, uint32_t* ri) {
    if (A.status[l] != PTX_OK) return 0u; /* only a log that is PTX_OK has runs */
    const uint64_t at = A.log_off[l];
    if (A.mark_type == PTX_MARK_COMMENT) {
        const ptx_cinterval* ci = A.cints + at;
        const uint64_t rows = A.log_off[l + 1u] - at;
        uint32_t n = A.logs[A.first_log + l].n_cintervals;
        if ((uint64_t)n > rows) n = (uint32_t)rows; /* (a result that is not this view's merge stays inside the log's rows) */
        uint32_t found = 0;
        for (uint32_t r0 = 0; r0 < n; r0 += 64u) {
            PTX_BALLOT64(hit, q0, (r0 + q0 < n && (A.id == PTX_MARK_ANY_ID || ci[r0 + q0].id == A.id)))
            if (kEmit) {
                PTX_FOR(q, 64u) {
                    const uint32_t slot = found + (uint32_t)__builtin_popcountll(hit & ((1ull << q) - 1ull));
                    if (((hit >> q) & 1ull) && slot < nl) {
                        const ptx_cinterval c = ci[r0 + q];
                        rs[slot] = c.start;
                        re[slot] = c.end;
                        ri[slot] = c.id;
                    }
                }
            }
            found += (uint32_t)__builtin_popcountll(hit);
            if ((kEmit && found >= nl) || n - r0 <= 64u) break;
        }
        return found;
    }
    const ptx_span* sp = A.spans + at;
    const uint32_t n = (uint32_t)(A.span_off[l + 1u] - A.span_off[l]);
    const uint32_t nv = ptx_markrun_visible(A, l);
    uint32_t starts = 0, ends = 0; /* of the steps before: the carry over a step's edge */
    for (uint32_t r0 = 0; r0 < n; r0 += 64u) {
        PTX_BALLOT64(sm, q0, (r0 + q0 < n && ptx_markrun_is_start(A, sp, r0 + q0)))
        PTX_BALLOT64(em, q1, (r0 + q1 < n && ptx_markrun_is_end(A, sp, n, r0 + q1)))
        if (kEmit) {
            PTX_FOR(q, 64u) {
                const uint64_t below = (1ull << q) - 1ull;
                const uint32_t i = r0 + q;
                if ((sm >> q) & 1ull) {
                    const uint32_t slot = starts + (uint32_t)__builtin_popcountll(sm & below);
                    if (slot < nl) {
                        const ptx_span row = sp[i];
                        rs[slot] = row.start;
                        ri[slot] = A.mark_type == PTX_MARK_LINK ? row.attr & PTX_ATTR_ID_MASK : 0u;
                    }
                }
                if ((em >> q) & 1ull) { /* the k-th end closes the k-th start: a listed run gets its end however many steps behind its start */
                    const uint32_t slot = ends + (uint32_t)__builtin_popcountll(em & below);
                    if (slot < nl) re[slot] = i + 1u < n ? sp[i + 1u].start : nv;
                }
            }
        }
        starts += (uint32_t)__builtin_popcountll(sm);
        ends += (uint32_t)__builtin_popcountll(em);
        if ((kEmit && ends >= nl) || n - r0 <= 64u) break; /* the cap: the listed runs are the FIRST nl, complete */
    }
    return starts;
}

template <uint32_t kThreads>
PTX_DEV void ptx_markrun_count_log(const PtxMarkRunArgs& A, uint32_t l) {
    const uint32_t n = ptx_markrun_walk<kThreads, false>(A, l, 0u, nullptr, nullptr, nullptr);
    PTX_LEADER {
        A.n_runs[l] = n;
        A.run_off[l] = n < A.cap ? n : A.cap;
        A.run_off[(uint64_t)(A.n_logs + 1u) + l] = 0ull; /* (the scan kernel scans two rows; the second is not used) */
    }
}

template <uint32_t kThreads>
PTX_DEV void ptx_markrun_emit_log(const PtxMarkRunArgs& A, uint32_t l) {
    const uint64_t o = A.run_off[l];
    const uint32_t nl = (uint32_t)(A.run_off[l + 1u] - o);
    if (nl != 0u) (void)ptx_markrun_walk<kThreads, true>(A, l, nl, A.run_start + o, A.run_end + o, A.run_id + o);
}

PTX_DEV void ptx_markrun_finish_one(const PtxMarkRunArgs& A, uint32_t k) {
    uint32_t lo = 0, hi = A.n_logs; /* the run's log: the LAST l with run_off[l] <= k (run_off[0] == 0 <= k < run_off[n_logs]) */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.run_off[mid] <= (uint64_t)k) lo = mid;
        else hi = mid;
    }
    const uint32_t l = lo;
    const uint32_t* pre = A.pre + A.pre_off[l];
    const uint32_t nv = ptx_markrun_visible(A, l); /* a log with a run is PTX_OK: it has n_visible + 1 words of prefix */
    const bool has = A.pre_off[l + 1u] != A.pre_off[l];
    const uint32_t s = A.run_start[k], e = A.run_end[k];
    const uint32_t cs = s < nv ? s : nv, ce = e < nv ? e : nv; /* (rows of a result that is not this view's merge stay inside the prefix) */
    const uint32_t us = has ? pre[cs] : 0u, ue = has ? pre[ce] : 0u;
    A.run_unit[k] = us;
    A.run_len[k] = ue > us ? ue - us : 0u;
    if (A.win_start) {
        const uint32_t ws = s > A.before ? s - A.before : 0u;
        const uint32_t we = e > 0xFFFFFFFFu - A.after ? 0xFFFFFFFFu : e + A.after;
        A.win_start[k] = ws;
        A.win_end[k] = we;
        const uint32_t a = ws < nv ? ws : nv; /* what ptx_slice_bounds_one makes of it: elem_start */
        A.match_unit[k] = has ? us - pre[a] : 0u;
    }
}

/* [hs, he) lies inside ONE of the n runs (disjoint, ascending by start): the last run with start <= hs decides */
PTX_DEV bool ptx_markrun_contains(const uint32_t* rs, const uint32_t* re, uint32_t n, uint32_t hs, uint32_t he) {
    uint32_t lo = 0, hi = n; /* runs with start <= hs */
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rs[mid] <= hs) lo = mid + 1u;
        else hi = mid;
    }
    return lo != 0u && he <= re[lo - 1u];
}

template <uint32_t kThreads, bool kEmit>
PTX_DEV void ptx_markrun_filter_log(const PtxMarkFilterArgs& A, uint32_t l) {
    const uint64_t h0 = A.hit_off[l], r0 = A.run_off[l];
    const uint32_t nh = (uint32_t)(A.hit_off[l + 1u] - h0), nr = (uint32_t)(A.run_off[l + 1u] - r0);
    const uint32_t *hs = A.hit_start + h0, *he = A.hit_end + h0, *rs = A.run_start + r0, *re = A.run_end + r0;
    const uint64_t o = kEmit ? A.out_off[l] : 0ull;
    const uint32_t nl = kEmit ? (uint32_t)(A.out_off[l + 1u] - o) : 0u;
    uint32_t kept = 0;
    if (nr != 0u && (!kEmit || nl != 0u)) {
        for (uint32_t k0 = 0; k0 < nh; k0 += 64u) {
            PTX_BALLOT64(in, q0, (k0 + q0 < nh && ptx_markrun_contains(rs, re, nr, hs[k0 + q0], he[k0 + q0])))
            if (kEmit) {
                PTX_FOR(q, 64u) {
                    const uint32_t slot = kept + (uint32_t)__builtin_popcountll(in & ((1ull << q) - 1ull));
                    if (((in >> q) & 1ull) && slot < nl) {
                        A.out_unit[o + slot] = A.hit_unit[h0 + k0 + q];
                        A.out_start[o + slot] = hs[k0 + q];
                        A.out_end[o + slot] = he[k0 + q];
                    }
                }
            }
            kept += (uint32_t)__builtin_popcountll(in);
            if ((kEmit && kept >= nl) || nh - k0 <= 64u) break;
        }
    }
    if (!kEmit) {
        PTX_LEADER A.n_kept[l] = kept;
    }
}
