/*
 * view_core.h — a resident text view: the assembled text and the element prefix of a range of logs of one merge, made once (ptx_text_view_create) and then
 * searched and cut any number of times (ptx_view_find_text, ptx_view_text_slices, ptx_view_find_snippets).
 *
 * The reference's caller keeps the string getTextWithFormatting returned (reference/src/peritext.ts:337-395) and runs indexOf and slice on it as often as it
 * likes.  ptx_result_find_text and ptx_result_text_slices re-assemble that string per call, and a slice call rebuilds the element prefix as well; the view keeps
 * both in device memory of its own:
 *
 *   status, text_off, span_off, text, span_unit   what text_core.h's passes leave for the range (ptx_result_text_range's answer, never downloaded)
 *   pre_off, pre                                  slice_core.h's exclusive element prefix pre[0 .. n_visible] of EVERY log that is PTX_OK, written by
 *                                                 ptx_slice_prefix_log itself: ptx_view_plan_one gives every log one slice (slice_off = 0, 1, 2, ...) and
 *                                                 plans n_visible + 1 words for every good log
 *   log_off                                       the batch's row offsets of the range: where a log's span rows start in the merge's result
 *
 * With the prefix resident a hit needs neither `values` nor the string table — which is what frees a query from the batch and from the strings:
 *
 *   ptx_find_count_log / ptx_find_positions_log   find_core.h's count walk and the position half of its emit walk, unchanged, over the view's text
 *   ptx_view_locate_one    a lane per listed hit, in place of find_core.h's tile walk.  Its log is the LAST one with hit_off[l] <= k (logs without hits are
 *                          passed over — the search of ptx_slice_bounds_one); two binary searches over the log's pre[0 .. n_visible): the holder of unit u is
 *                          the LAST element e < n_visible with pre[e] <= u (ptx_find_holder: an empty string before the holder has an equal pre and is passed
 *                          over, one behind it has pre > u; pre[n_visible] is never read).  hit_start = holder(hit_unit), hit_end = holder(hit_unit + m - 1) + 1
 *   ptx_view_windows_one   a lane per listed hit: [hit_start - before, hit_end + after), the subtraction saturating at 0, the addition at 0xFFFFFFFF, into the
 *                          arrays the slice passes read as slice_start / slice_end (slice_off is hit_off: one snippet per hit, in hit order).  The pass clamps
 *                          the start itself — hit_start < n_visible, so min(start, n_visible) is the start — and with that writes
 *                          match_unit = hit_unit - pre[start]: where the match sits inside the snippet's text.  No pass of its own is needed for it.
 *   (ptx_slice_bounds_one, the offsets scan, ptx_slice_copy_block and ptx_slice_span_one run unchanged on these device-resident bounds)
 *
 * Plain vector loads and stores only; written against the platform layer like the other cores: hipcc builds it into the product, tests/emu/emu_view.cc plays it
 * on one host thread.
 */
#pragma once
#include "find_core.h"
#include "slice_core.h"

struct PtxViewArgs {
    PtxFindArgs F;           /* T.n_logs, hit_off, hit_unit, hit_start, hit_end, n_pattern: the hits */
    const uint64_t* pre_off; /* the view's [n_logs + 1] */
    const uint32_t* pre;     /* ... [pre_off[n_logs]] */
    uint32_t n_hits;         /* hit_off[n_logs] */
    uint32_t before, after, pad;
    uint32_t* win_start;     /* [n_hits] the slice passes' slice_start */
    uint32_t* win_end;       /* ... slice_end */
    uint32_t* match_unit;    /* [n_hits] */
};

/* the plan of a view, a lane per log: EVERY log has one slice as far as ptx_slice_prefix_log is concerned, and every good one n_visible + 1 words of `pre` */
PTX_DEV void ptx_view_plan_one(const PtxSliceArgs& A, uint64_t* every_log /* [n_logs + 1], becomes A.slice_off */, uint32_t l) {
    every_log[l] = l;
    if (l + 1u == A.T.n_logs) every_log[l + 1u] = (uint64_t)l + 1u;
    A.pre_off[l] = A.T.status[l] == PTX_OK ? (uint64_t)ptx_slice_visible(A, l) + 1u : 0ull;
    A.pre_off[(uint64_t)(A.T.n_logs + 1u) + l] = 0ull; /* (the scan kernel scans two rows; the second is not used) */
}

/* the log of listed hit k: the LAST l with hit_off[l] <= k (hit_off[0] == 0 <= k < hit_off[n_logs]) */
PTX_DEV uint32_t ptx_view_log_of(const PtxViewArgs& A, uint32_t k) {
    uint32_t lo = 0, hi = A.F.T.n_logs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.F.hit_off[mid] <= (uint64_t)k) lo = mid;
        else hi = mid;
    }
    return lo;
}

PTX_DEV void ptx_view_locate_one(const PtxViewArgs& A, uint32_t k) {
    const uint32_t l = ptx_view_log_of(A, k);
    const uint32_t* pre = A.pre + A.pre_off[l];
    const uint32_t words = (uint32_t)(A.pre_off[l + 1u] - A.pre_off[l]); /* n_visible + 1: a log with a hit has text, so it is PTX_OK and has an element */
    const uint32_t nv = words ? words - 1u : 0u;
    const uint32_t u = A.F.hit_unit[k];
    uint32_t s = 0, e = 0;
    if (nv) { /* (a view that is not this result's gets the log's start, not a read outside its prefix) */
        s = ptx_find_holder(pre, nv, u);
        e = ptx_find_holder(pre, nv, u + (A.F.n_pattern - 1u)) + 1u; /* (u + m - 1 < L < 2^32: no wrap) */
    }
    A.F.hit_start[k] = s;
    A.F.hit_end[k] = e;
}

PTX_DEV void ptx_view_windows_one(const PtxViewArgs& A, uint32_t k) {
    const uint32_t l = ptx_view_log_of(A, k);
    const uint32_t words = (uint32_t)(A.pre_off[l + 1u] - A.pre_off[l]);
    const uint32_t nv = words ? words - 1u : 0u;
    const uint32_t hs = A.F.hit_start[k], he = A.F.hit_end[k];
    const uint32_t ws = hs > A.before ? hs - A.before : 0u;
    const uint32_t we = he > 0xFFFFFFFFu - A.after ? 0xFFFFFFFFu : he + A.after;
    A.win_start[k] = ws;
    A.win_end[k] = we;
    const uint32_t a = ws < nv ? ws : nv; /* what ptx_slice_bounds_one makes of it: elem_start */
    A.match_unit[k] = words ? A.F.hit_unit[k] - A.pre[A.pre_off[l] + a] : 0u;
}
