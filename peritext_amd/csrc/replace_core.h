/*
 * replace_core.h — find and replace on a resident text view: the hits of a pattern made into the InputOperations that replace them (ptx_view_replace_plan).
 *
 * The reference's editor turns a ProseMirror ReplaceStep into a `delete` followed by an `insert` at the same index (reference/src/bridge.ts:425-446); what is
 * pinned here is String.prototype.replaceAll(pattern, ...) over the text getTextWithFormatting returns (reference/src/peritext.ts:337-395): of ALL matches of a
 * log — find_core.h's, overlapping ones included — the greedy, leftmost, non-overlapping ones are CHOSEN: the first match, and after a chosen match at unit u
 * the first with hit_unit >= u + m.  The choice does not look at elements.  A chosen match is REPLACEABLE iff it covers whole elements,
 * pre[hit_start] == hit_unit and pre[hit_end] == hit_unit + m over the view's resident prefix; one that starts or ends inside a multi-unit element is counted
 * and skipped, and still blocks the matches it overlaps.
 *
 * The hits are the view's: ptx_find_count_log, the scan, ptx_find_positions_log and ptx_view_locate_one, unchanged, with no cap.  Then
 *
 *   ptx_replace_select_log   ONE 64-lane wave per log, as the count and positions passes.  It walks the log's hits in tiles of PTX_REPLACE_TILE = 64, a lane per
 *                            hit, and carries `limit`: the unit behind the last chosen match.  Inside a tile the chosen hits are ONE chain: it starts at the
 *                            first hit with hit_unit >= limit (a ballot) and follows next(i) = the first j of the tile with unit[j] >= unit[i] + m (a binary
 *                            search of every lane over the tile's units in LDS; 64 = "leaves the tile").  The chain is marked by pointer doubling: six
 *                            rounds of { a marked hit marks jump[i]; jump[i] = jump[jump[i]] }, the jumps ping-ponging between two LDS arrays — after
 *                            round r the hits at chain distance < 2^(r+1) of the start are marked, after six all 64.  No lane ever walks hits one after the
 *                            other: "aaaa..." under "aa" is a chain as long as the document and costs what any other tile costs.  A mark is only ever set
 *                            on a hit of the chain, so a lane that sees a mark of its own round early changes nothing.  The last chosen hit of the tile
 *                            sets the carried limit.  Two ballots — chosen, replaceable — give the counts and the rank r of a replaced hit among the log's
 *                            replaced hits in scalar registers.  Written: sel[k] = 0 not chosen / 1 chosen but inside an element / 2 + r replaced; per log
 *                            n_chosen, n_replaced, the plan's status, n_ops, and makes[first_log + l] = "this log makes a Change".
 *   (the host library scans `makes` over n_batch_logs into chg_off and n_ops over the view's logs into op_log_off: ptx_find_offsets_kernel, twice)
 *   ptx_replace_emit_one     a lane per hit: a replaced hit of rank r of a log with R of them writes its k = 1 or 2 ops at op_log_off[l] + (R - 1 - r) * k —
 *                            DESCENDING hit order, so no index needs adjusting —: PTX_IN_DELETE {hit_start, hit_end - hit_start} and, with a replacement,
 *                            PTX_IN_INSERT {hit_start, n_replacement, payload 0}.  The hit of rank 0 also writes its Change's op_off entry (the Changes are
 *                            the logs with ops, in order: op_off[chg_off[first_log + l]] = op_log_off[l]), the last Change's its end.
 *
 * Rows of a log's Change = the deleted elements + R * n_replacement; more than PTX_CHANGE_ROWS_MAX is PTX_ERR_CAPACITY for that log: no ops, the counts stay.
 *
 * Plain vector loads and stores only; written against the platform layer like the other cores: hipcc builds it into the product, tests/emu/emu_replace.cc plays
 * it on one host thread.
 */
#pragma once
#include "view_core.h"

#define PTX_REPLACE_TILE 64u /* hits of a step of the select walk: a lane each (mirrored in peritext_amd/abi.py: the tests take their edge sizes from it) */

struct PtxReplaceArgs {
    PtxViewArgs V;           /* F.T.n_logs, F.T.status, F.hit_off, F.hit_unit, F.hit_start, F.hit_end, F.n_pattern, pre_off, pre, n_hits */
    uint32_t n_replacement, first_log, n_batch_logs, pad;
    uint32_t* sel;           /* [n_hits] 0 | 1 | 2 + rank among the log's replaced hits */
    uint32_t* status;        /* [n_logs] the plan's: the view's, or PTX_ERR_CAPACITY */
    uint32_t* n_chosen;      /* [n_logs] */
    uint32_t* n_replaced;    /* [n_logs] */
    uint32_t* n_ops;         /* [n_logs] InputOperations the log makes: 0 for a log that is not PTX_OK */
    uint32_t* makes;         /* [n_batch_logs] zeroed by the host; 1 where a log makes a Change */
    uint64_t* chg_off;       /* [n_batch_logs + 1] the scan of makes */
    uint64_t* op_log_off;    /* [n_logs + 1] the scan of n_ops */
    uint64_t* op_off;        /* [n_changes + 1] */
    uint8_t* action;         /* [n_input_ops] ... */
    uint8_t* mark_type;
    uint32_t* index;
    uint32_t* count;
    uint32_t* payload;
};

struct PtxReplaceHdr {
    uint32_t del; /* elements the log's replaced matches delete */
    uint32_t pad[7];
};
/* LDS of a wave: header | the tile's hit units | marks | jumps (two arrays); entry 64 of the last three is "behind the tile" */
#define PTX_REPLACE_LDS_UNIT 32u
#define PTX_REPLACE_LDS_MARK (PTX_REPLACE_LDS_UNIT + 4u * PTX_REPLACE_TILE)
#define PTX_REPLACE_LDS_JUMP (PTX_REPLACE_LDS_MARK + 80u)
#define PTX_REPLACE_LDS_BYTES (PTX_REPLACE_LDS_JUMP + 2u * 80u)
static_assert(sizeof(PtxReplaceHdr) == PTX_REPLACE_LDS_UNIT, "the header fills the first 32 bytes of a wave's LDS");
static_assert(PTX_REPLACE_TILE == 64u, "a lane per hit of the tile, a bit per hit in the ballots, six rounds of doubling");

/* the first j in (q, nt) with un[j] >= want, 64 if there is none: the units ascend strictly */
PTX_DEV uint32_t ptx_replace_next(const uint32_t* un, uint32_t nt, uint32_t q, uint32_t want) {
    uint32_t lo = q, hi = nt; /* un[lo] < want <= un[hi] (hi == nt: none) */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (un[mid] < want) lo = mid;
        else hi = mid;
    }
    return hi < nt ? hi : PTX_REPLACE_TILE;
}

/* does hit k = [u, u + m) of a log with the prefix pre[0 .. words) cover whole elements? */
PTX_DEV bool ptx_replace_whole(const PtxReplaceArgs& A, const uint32_t* pre, uint32_t words, uint64_t k, uint32_t u) {
    const uint32_t s = A.V.F.hit_start[k], e = A.V.F.hit_end[k];
    if (s >= words || e >= words) return false; /* (a view that is not this result's: nothing is read outside the prefix) */
    return pre[s] == u && pre[e] == u + A.V.F.n_pattern;
}

template <uint32_t kThreads>
PTX_DEV void ptx_replace_select_log(const PtxReplaceArgs& A, uint32_t l, uint8_t* lds) {
    PtxReplaceHdr* H = (PtxReplaceHdr*)lds;
    uint32_t* un = (uint32_t*)(lds + PTX_REPLACE_LDS_UNIT);
    uint8_t* mark = lds + PTX_REPLACE_LDS_MARK;
    uint8_t* jump0 = lds + PTX_REPLACE_LDS_JUMP;
    uint8_t* jump1 = jump0 + 80u;
    const uint64_t h0 = A.V.F.hit_off[l];
    const uint32_t nh = (uint32_t)(A.V.F.hit_off[l + 1u] - h0);
    const uint32_t m = A.V.F.n_pattern;
    const uint32_t* hu = A.V.F.hit_unit + h0;
    const uint32_t* pre = A.V.pre + A.V.pre_off[l];
    const uint32_t words = (uint32_t)(A.V.pre_off[l + 1u] - A.V.pre_off[l]);
    PTX_LEADER H->del = 0;
    uint32_t limit = 0;      /* the unit behind the last chosen match */
    uint32_t nc = 0, nr = 0; /* chosen, replaced so far */
    for (uint32_t t0 = 0; t0 < nh; t0 += PTX_REPLACE_TILE) {
        const uint32_t nt = nh - t0 < PTX_REPLACE_TILE ? nh - t0 : PTX_REPLACE_TILE;
        PTX_SYNC_T(); /* the header is written; the tile before has been read */
        PTX_FOR(q, nt) un[q] = hu[t0 + q];
        PTX_LEADER mark[PTX_REPLACE_TILE] = 0, jump0[PTX_REPLACE_TILE] = jump1[PTX_REPLACE_TILE] = (uint8_t)PTX_REPLACE_TILE;
        PTX_SYNC_T();
        PTX_BALLOT64(free_, q0, (q0 < nt && un[q0] >= limit))
        const uint32_t start = free_ ? (uint32_t)__builtin_ctzll(free_) : PTX_REPLACE_TILE; /* the head of the tile's chain */
        PTX_FOR(q, PTX_REPLACE_TILE) {
            mark[q] = q == start ? 1u : 0u;
            jump0[q] = (uint8_t)(q < nt ? ptx_replace_next(un, nt, q, un[q] + m) : PTX_REPLACE_TILE); /* (un + m <= the text's length < 2^32: no wrap) */
        }
        for (uint32_t r = 0; r < 6u; ++r) { /* after round r the chain's hits at distance < 2^(r+1) of the head are marked, and a jump is 2^(r+1) links */
            const uint8_t* from = (r & 1u) ? jump1 : jump0;
            uint8_t* to = (r & 1u) ? jump0 : jump1;
            PTX_SYNC_T();
            PTX_FOR(q, PTX_REPLACE_TILE) {
                const uint32_t j = from[q];
                if (mark[q]) mark[j] = 1u; /* (only ever a hit of the chain: one seen a round early marks what a later round would) */
                to[q] = from[j];
            }
        }
        PTX_SYNC_T();
        PTX_BALLOT64(chosen, q1, (q1 < nt && mark[q1] != 0u))
        PTX_BALLOT64(whole, q2, (q2 < nt && mark[q2] != 0u && ptx_replace_whole(A, pre, words, h0 + t0 + q2, un[q2])))
        PTX_GEN_FOR(q, PTX_REPLACE_TILE) {
            uint32_t d = 0;
            if (q < nt) {
                const uint64_t k = h0 + t0 + q;
                const bool w = ((whole >> q) & 1ull) != 0ull;
                A.sel[k] = w ? 2u + nr + (uint32_t)__builtin_popcountll(whole & ((1ull << q) - 1ull)) : (uint32_t)((chosen >> q) & 1ull);
                if (w) d = A.V.F.hit_end[k] - A.V.F.hit_start[k];
            }
            ptx_reduce_add32(&H->del, d); /* (matches that cover whole elements and do not overlap: the sum is at most n_visible) */
        }
        if (chosen) limit = PTX_U32(un[63u - (uint32_t)__builtin_clzll(chosen)]) + m; /* the chain leaves the tile */
        nc += (uint32_t)__builtin_popcountll(chosen);
        nr += (uint32_t)__builtin_popcountll(whole);
    }
    PTX_SYNC_T();
    PTX_LEADER {
        const uint64_t rows = (uint64_t)H->del + (uint64_t)nr * A.n_replacement;
        uint32_t st = A.V.F.T.status[l];
        if (st == PTX_OK && rows > PTX_CHANGE_ROWS_MAX) st = PTX_ERR_CAPACITY;
        const uint32_t ops = st == PTX_OK ? nr * (A.n_replacement ? 2u : 1u) : 0u; /* (nr <= rows <= 65 534 here) */
        A.status[l] = st;
        A.n_chosen[l] = nc;
        A.n_replaced[l] = nr;
        A.n_ops[l] = ops;
        A.makes[A.first_log + l] = ops ? 1u : 0u;
    }
}

PTX_DEV void ptx_replace_emit_one(const PtxReplaceArgs& A, uint32_t k) {
    const uint32_t w = A.sel[k];
    if (w < 2u) return;
    const uint32_t l = ptx_view_log_of(A.V, k);
    if (A.n_ops[l] == 0u) return; /* a log beyond the capacity makes no ops */
    const uint32_t r = w - 2u, R = A.n_replaced[l], per = A.n_replacement ? 2u : 1u;
    const uint64_t base = A.op_log_off[l];
    const uint64_t at = base + (uint64_t)(R - 1u - r) * per;
    const uint32_t s = A.V.F.hit_start[k];
    A.action[at] = (uint8_t)PTX_IN_DELETE;
    A.mark_type[at] = 0;
    A.index[at] = s;
    A.count[at] = A.V.F.hit_end[k] - s;
    A.payload[at] = 0;
    if (per == 2u) { /* bridge.ts:425-446: the delete, then the insert at the same index */
        A.action[at + 1u] = (uint8_t)PTX_IN_INSERT;
        A.mark_type[at + 1u] = 0;
        A.index[at + 1u] = s;
        A.count[at + 1u] = A.n_replacement;
        A.payload[at + 1u] = 0; /* every insert shares the caller's n_replacement value ids */
    }
    if (r == 0u) {
        const uint64_t c = A.chg_off[A.first_log + l];
        A.op_off[c] = base;
        if (c + 1u == A.chg_off[A.n_batch_logs]) A.op_off[c + 1u] = A.op_log_off[A.V.F.T.n_logs];
    }
}
