/*
 * slice_core.h — the text and the span rows of many ranges of visible ELEMENT indexes of resident documents (ptx_result_text_slices).
 *
 * The reference's caller slices the text getTextWithFormatting returned (reference/src/peritext.ts:337-395).  Here the ranges come up — hits of find_core.h
 * widened by some context, comment intervals, a viewport — and a few kilobytes come down.  What is pinned is Array.prototype.slice(start, end) over a log's
 * n_visible elements for non-negative arguments; the spans are the log's rows clipped to the range, `start` still a document element index.
 *
 * The text is the one text_core.h assembles (lengths, offsets, assemble: unchanged) into a pool block that never leaves the device.  Then:
 *
 *   ptx_slice_prefix_log   ONE 64-lane wave per log (text_core.h says why), and only for a log that has a slice: the tile walk of the assemble pass — ids ->
 *                          lengths, one wave-wide exclusive scan, the carry in a register — written out as pre[0 .. n_visible] (u32, exclusive) into a scratch
 *                          block.  text_core.h keeps no per-element prefix in HBM because span starts are sorted and a forward cursor serves them; slice bounds
 *                          come unsorted and in any number, so here it exists: 4 bytes per visible element (+ 4) of the logs that have slices, and a bound is
 *                          one gather.
 *   ptx_slice_bounds_one   a lane per slice.  Its log is the LAST one with slice_off[l] <= k (logs without slices are passed over); clamp; len = pre[b] - pre[a];
 *                          two binary searches over the log's span rows (sorted by start) give the first row (the last with start <= a) and one past the last
 *                          (the first with start >= b).  elem_start, elem_end, the unit length and the row count go out, and for the two passes below the log,
 *                          the first row and the source offset of the slice's first unit in the assembled text.
 *   (the host library scans lengths and row counts into unit_off / sspan_off with ptx_text_offsets_kernel, one launch for both rows)
 *   ptx_slice_copy_block   balanced over OUTPUT: one wave per PTX_SLICE_BLOCK code units of it, whether they are one stretch of a 100 000-unit viewport or thirty
 *                          snippets.  ONE uniform binary search over unit_off finds the LAST slice with unit_off <= block start — runs of empty slices are
 *                          passed over —; from there the slice boundaries are staged 64 at a time into LDS, and every lane finds the slice of its unit among
 *                          them (six steps in LDS) and copies text[src_off[k] + (u - unit_off[k])].  Source and destination parities are independent:
 *                          2-byte loads and stores, consecutive lanes on consecutive units.
 *   ptx_slice_span_one     a lane per output row: the same search over sspan_off, the log's row first_span[k] + j, its start raised to elem_start,
 *                          sspan_unit = pre[start] - pre[elem_start].
 *
 * Plain vector loads and stores only; written against the platform layer like the other cores: hipcc builds it into the product, tests/emu/emu_slice.cc plays it
 * on one host thread.
 */
#pragma once
#include "text_core.h"

#define PTX_SLICE_BLOCK 1024u /* code units of the output that one wave of the copy pass writes (mirrored in peritext_amd/abi.py: the tests take their edge sizes from it) */
#define PTX_SLICE_CHUNK 64u   /* slice boundaries staged per step of the copy pass: a lane each */

struct PtxSliceArgs {
    PtxTextArgs T;              /* the text passes' arguments: status, off (text_off | span_off), text, and what the element walk reads */
    const uint64_t* slice_off;  /* device [n_logs + 1] */
    const uint32_t* slice_start; /* device [n_slices] */
    const uint32_t* slice_end;
    uint32_t n_slices, pad;
    uint64_t* pre_off;          /* [2][n_logs + 1]: row 0 = where a log's prefix starts in `pre` (the plan leaves n_visible + 1 or 0 there, the host's scan sums it) */
    uint32_t* pre;              /* [pre_off[n_logs]] */
    uint32_t* elem_start;       /* [n_slices] */
    uint32_t* elem_end;
    uint64_t* out_off;          /* [2][n_slices + 1]: unit lengths | row counts from the bounds pass, scanned in place into unit_off | sspan_off */
    uint32_t* slice_log;        /* [n_slices] scratch: the slice's log within the range */
    uint32_t* first_span;       /* [n_slices] scratch: the first of the log's span rows that reaches into the slice */
    uint64_t* src_off;          /* [n_slices] scratch: the slice's first unit in T.text */
    uint16_t* out_text;         /* [unit_off[n_slices]] */
    ptx_span* out_spans;        /* [sspan_off[n_slices]] */
    uint32_t* out_span_unit;
};

struct PtxSliceHdr {
    uint32_t run; /* prefix: cursor of the tile's scan */
    uint32_t end; /* ... the scan value behind the tile's last element */
    uint32_t pad[6];
};
/* LDS of a wave of the copy pass: the staged unit_off of up to PTX_SLICE_CHUNK slices and the one behind them | their source offsets */
#define PTX_SLICE_LDS_SRC ((8u * (PTX_SLICE_CHUNK + 1u) + 15u) & ~15u)
#define PTX_SLICE_LDS_BYTES (PTX_SLICE_LDS_SRC + 8u * PTX_SLICE_CHUNK)
static_assert(sizeof(PtxSliceHdr) == 32u && sizeof(PtxSliceHdr) <= PTX_SLICE_LDS_BYTES, "the prefix pass's header fits the block both passes declare");

/* visible elements of log l of the range that a slice can reach: none of a log that has no text */
PTX_DEV uint32_t ptx_slice_visible(const PtxSliceArgs& A, uint32_t l) {
    if (A.T.logs == nullptr) { /* a query of a resident view (view_core.h) has no per-log rows: its prefix holds n_visible + 1 words for every good log, none for another */
        const uint64_t words = A.pre_off[l + 1u] - A.pre_off[l];
        return words ? (uint32_t)words - 1u : 0u;
    }
    const uint32_t log = A.T.first_log + l;
    return A.T.status[l] == PTX_OK ? ptx_text_rows(A.T, log, A.T.logs[log].n_visible) : 0u;
}

/* the plan, a lane per log: the words of `pre` the log needs — n_visible + 1 where it has a slice and a text */
PTX_DEV void ptx_slice_plan_one(const PtxSliceArgs& A, uint32_t l) {
    const bool need = A.slice_off[l + 1u] != A.slice_off[l] && A.T.status[l] == PTX_OK;
    A.pre_off[l] = need ? (uint64_t)ptx_slice_visible(A, l) + 1u : 0ull;
    A.pre_off[(uint64_t)(A.T.n_logs + 1u) + l] = 0ull; /* (the scan kernel scans two rows; the second is not used) */
}

template <uint32_t kThreads>
PTX_DEV void ptx_slice_prefix_log(const PtxSliceArgs& A, uint32_t l, uint8_t* lds) {
    PtxSliceHdr* H = (PtxSliceHdr*)lds;
    if (A.slice_off[l + 1u] == A.slice_off[l] || A.T.status[l] != PTX_OK) return; /* a log without a slice, or without text: no words of `pre` are its */
    const uint32_t log = A.T.first_log + l;
    const uint32_t nv = ptx_slice_visible(A, l);
    const uint32_t* vals = A.T.values + A.T.log_off[log];
    uint32_t* pre = A.pre + A.pre_off[l];
    uint32_t carry = 0; /* units before the tile */
    for (uint32_t t0 = 0; t0 < nv; t0 += PTX_TEXT_TILE) {
        const uint32_t nt = nv - t0 < PTX_TEXT_TILE ? nv - t0 : PTX_TEXT_TILE;
        PTX_LEADER H->run = 0;
        PTX_SYNC_T();
        PTX_GEN_FOR(lane, 64u) { /* the scan of text_core.h's assemble pass */
            const uint32_t e0 = lane * PTX_TEXT_PER_LANE;
            uint32_t ln[PTX_TEXT_PER_LANE], cnt = 0;
            for (uint32_t j = 0; j < PTX_TEXT_PER_LANE; ++j) {
                ln[j] = 0;
                if (e0 + j < nt) {
                    const uint32_t id = vals[t0 + e0 + j]; /* < n_strings: the length pass has seen every id of a log whose status is PTX_OK */
                    ln[j] = (uint32_t)(A.T.str_off[id + 1u] - A.T.str_off[id]);
                }
                cnt += ln[j];
            }
            uint32_t p = carry + ptx_append_n(&H->run, cnt);
            for (uint32_t j = 0; j < PTX_TEXT_PER_LANE; ++j) {
                if (e0 + j < nt) pre[t0 + e0 + j] = p;
                p += ln[j];
            }
            if (e0 < nt && e0 + PTX_TEXT_PER_LANE >= nt) H->end = p; /* the lane of the tile's last element: the tile's end */
        }
        PTX_SYNC_T();
        carry = PTX_U32(H->end);
        PTX_SYNC_T(); /* the next tile rewrites the header */
    }
    PTX_LEADER pre[nv] = carry; /* == the log's text length */
}

/* rows of sp[0 .. n) with start < x (kLess) / start <= x: the rows are sorted by start */
template <bool kLess>
PTX_DEV uint32_t ptx_slice_rows_before(const ptx_span* sp, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t st = sp[mid].start;
        if (kLess ? st < x : st <= x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

PTX_DEV void ptx_slice_bounds_one(const PtxSliceArgs& A, uint32_t k) {
    uint32_t lo = 0, hi = A.T.n_logs; /* the slice's log: the LAST l with slice_off[l] <= k (slice_off[0] == 0 <= k < slice_off[n_logs]) */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.slice_off[mid] <= (uint64_t)k) lo = mid;
        else hi = mid;
    }
    const uint32_t l = lo, log = A.T.first_log + l;
    const uint32_t nv = ptx_slice_visible(A, l);
    const uint32_t s = A.slice_start[k], e = A.slice_end[k];
    uint32_t a = s < nv ? s : nv, b = e < nv ? e : nv;
    if (a >= b) b = a; /* the empty slice stands at min(start, n_visible); of a log without text at 0 */
    uint32_t len = 0, first = 0, rows = 0;
    uint64_t src = 0;
    if (a < b) {
        const uint32_t* pre = A.pre + A.pre_off[l];
        const uint64_t* span_off = A.T.off + (uint64_t)(A.T.n_logs + 1u);
        const ptx_span* sp = A.T.spans + A.T.log_off[log];
        const uint32_t ns = (uint32_t)(span_off[l + 1u] - span_off[l]);
        len = pre[b] - pre[a];
        src = A.T.off[l] + pre[a];
        const uint32_t upto_a = ptx_slice_rows_before<false>(sp, ns, a); /* rows with start <= a: the last of them holds element a */
        const uint32_t below_b = ptx_slice_rows_before<true>(sp, ns, b);
        first = upto_a ? upto_a - 1u : 0u; /* (a merge's first row starts at element 0; one that does not is raised to a like any first row) */
        rows = below_b > first ? below_b - first : 0u;
    }
    A.elem_start[k] = a;
    A.elem_end[k] = b;
    A.out_off[k] = len;
    A.out_off[(uint64_t)A.n_slices + 1u + k] = rows;
    A.slice_log[k] = l;
    A.first_span[k] = first;
    A.src_off[k] = src;
}

template <uint32_t kThreads>
PTX_DEV void ptx_slice_copy_block(const PtxSliceArgs& A, uint32_t blk, uint8_t* lds) {
    uint64_t* bnd = (uint64_t*)lds;
    uint64_t* src = (uint64_t*)(lds + PTX_SLICE_LDS_SRC);
    const uint32_t n = A.n_slices;
    const uint64_t total = A.out_off[n];
    const uint64_t u0 = (uint64_t)blk * PTX_SLICE_BLOCK;
    if (u0 >= total) return;
    const uint64_t u1 = total - u0 < PTX_SLICE_BLOCK ? total : u0 + PTX_SLICE_BLOCK;
    uint32_t lo = 0, hi = n; /* the LAST slice with unit_off <= u0: it is not empty (unit_off[lo + 1] > u0), the empty ones before it are passed over */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.out_off[mid] <= u0) lo = mid;
        else hi = mid;
    }
    for (uint32_t k = lo;;) {
        const uint32_t nk = n - k < PTX_SLICE_CHUNK ? n - k : PTX_SLICE_CHUNK;
        PTX_SYNC_T(); /* the chunk before has been read */
        PTX_FOR(q, nk + 1u) {
            bnd[q] = A.out_off[k + q];
            if (q < nk) src[q] = A.src_off[k + q];
        }
        PTX_SYNC_T();
        const uint64_t b0 = bnd[0], b1 = bnd[nk];
        const uint64_t c0 = b0 > u0 ? b0 : u0, c1 = b1 < u1 ? b1 : u1; /* the chunk's units inside the block: bnd[0] <= c0 <= c1 <= bnd[nk] */
        PTX_FOR(i, c1 > c0 ? (uint32_t)(c1 - c0) : 0u) {
            const uint64_t u = c0 + i;
            uint32_t x = 0, y = nk; /* the slice that holds u: the last q < nk with bnd[q] <= u */
            while (y - x > 1u) {
                const uint32_t mid = (x + y) >> 1;
                if (bnd[mid] <= u) x = mid;
                else y = mid;
            }
            A.out_text[u] = A.T.text[src[x] + (u - bnd[x])];
        }
        if (b1 >= u1 || k + nk >= n) break;
        k += nk;
    }
}

PTX_DEV void ptx_slice_span_one(const PtxSliceArgs& A, uint64_t r) {
    const uint64_t* sspan_off = A.out_off + (uint64_t)A.n_slices + 1u;
    uint32_t lo = 0, hi = A.n_slices; /* the row's slice: the LAST k with sspan_off[k] <= r */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sspan_off[mid] <= r) lo = mid;
        else hi = mid;
    }
    const uint32_t k = lo, l = A.slice_log[k], a = A.elem_start[k];
    const uint32_t* pre = A.pre + A.pre_off[l];
    const ptx_span row = A.T.spans[A.T.log_off[A.T.first_log + l] + A.first_span[k] + (uint32_t)(r - sspan_off[k])];
    const uint32_t b = A.elem_end[k];
    uint32_t start = row.start > a ? row.start : a; /* only the slice's first row can start before it */
    if (start > b) start = b;                       /* (rows that are not sorted — a result that is not this batch's merge — stay inside the prefix) */
    A.out_spans[r] = ptx_span{start, row.attr};
    A.out_span_unit[r] = pre[start] - pre[a];
}
