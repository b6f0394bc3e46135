/*
 * text_core.h — document text on the device: the value ids a merge left behind, turned into ONE UTF-16 buffer per downloaded range (ptx_result_text_range).
 *
 * getTextWithFormatting returns {text, marks}[] (reference/src/peritext.ts:337-395; addCharactersToSpans :438-455 appends a character's value to its span's
 * text).  The merge produces value IDS and spans whose `start` is an ELEMENT index; a value is any JS string — one character as the editor types it, a pasted
 * paragraph as one insert (test/micromerge.ts:202), the empty string, half of a surrogate pair — so element indexes are not text offsets.  Two passes over the
 * logs of a range, both ONE 64-lane wave per log:
 *
 *   ptx_text_length_log    sum of len(string[values[i]]) over the log's n_visible elements, read where the merge wrote them (row log_off[l] of `values`).  Every
 *                          id is checked against the table here, BEFORE anything is read through it: an id >= n_strings makes the log PTX_ERR_BAD_OP, a text
 *                          of 2^32 code units or more PTX_ERR_CAPACITY, a log the merge failed keeps its merge status; such a log has no text.  The host scans
 *                          the lengths (and the span counts) into text_off / span_off.
 *   ptx_text_assemble_log  walks the visible elements in tiles of PTX_TEXT_TILE = 64 lanes x PTX_TEXT_PER_LANE consecutive elements.  Per tile: a lane loads its
 *                          ids, looks up (offset, length) in the table, one wave-wide exclusive scan of the lanes' lengths (carried from tile to tile in a
 *                          register) gives every element's code-unit offset; those go to LDS with the source offsets.  Then the copy:
 *                            - every value of the tile one unit long (what an editor produces): a lane's four units are one contiguous 8-byte run of the
 *                              output, written as two dword stores where it starts on an even unit and as unit / dword / unit where it starts on an odd one (a
 *                              log's text starts wherever the one before ended); the elements of a tile's ragged end go unit by unit;
 *                            - otherwise a value of up to PTX_TEXT_LANE_MAX units is copied by its lane, a longer one is listed in LDS and copied by the
 *                              whole wave, consecutive lanes on consecutive units.
 *                          span_unit[k] = the scan value at element spans[k].start, read from the tile's scan in LDS in the same pass: spans are sorted by
 *                          start, so a cursor over them moves forward tile by tile.  No per-element prefix array ever exists in HBM.
 *
 * Why a wave per log and not a workgroup: a document that holds text has a few thousand visible elements (a 4 096-op `rich4k` log keeps ~1 900), a range has
 * thousands of logs — the logs, not the lanes of one log, fill the machine; a wave's scan is one DPP prefix sum, its phases are separated by its own program
 * order (no s_barrier), and 3.6 KB of LDS per wave never bound the waves a CU holds.
 *
 * Written against the platform layer like the other cores: hipcc builds it into the product, tests/emu/emu_text.cc plays it on one host thread.
 */
#pragma once
#include "merge_core.h"

#define PTX_TEXT_PER_LANE 4u                       /* consecutive elements of a lane */
#define PTX_TEXT_TILE (64u * PTX_TEXT_PER_LANE)    /* elements per step of the walk (mirrored in peritext_amd/abi.py: the tests take their edge sizes from it) */
#define PTX_TEXT_LANE_MAX 16u                      /* a value of up to this many code units is copied by its own lane, a longer one by the whole wave */

struct PtxTextArgs {
    const uint64_t* log_off;       /* the batch's */
    const ptx_log_result* logs;    /* the merge's per-log rows */
    const uint32_t* values;        /* ... value ids, a log's at row log_off[l] */
    const ptx_span* spans;         /* ... spans, likewise */
    const uint16_t* units;         /* the string table: code units back to back */
    const uint64_t* str_off;       /* [n_strings + 1] */
    uint32_t n_strings;
    uint32_t first_log, n_logs;    /* the range */
    uint32_t* status;              /* [n_logs] */
    uint64_t* off;                 /* [2][n_logs + 1]: the length pass leaves the code units / spans of log l at [0][l] / [1][l]; the host's scan turns both rows
                                      into exclusive prefix sums in place: text_off, span_off */
    uint16_t* text;                /* [text_off[n_logs]] */
    uint32_t* span_unit;           /* [span_off[n_logs]] */
};

struct PtxTextHdr {
    unsigned long long sum; /* length pass: code units of the log */
    uint32_t bad;           /* ... 1: an id beyond the table, 2: a value of 2^32 units or more */
    uint32_t run;           /* assemble: cursor of the tile's scan */
    uint32_t not_one;       /* ... some value of the tile is not exactly one unit long */
    uint32_t n_long;        /* ... values of the tile the whole wave copies */
    uint32_t pad[2];
};
/* LDS of a wave: header | unit offset of every element of the tile within the log's text, and the tile's end | source offset of every element | the long values */
#define PTX_TEXT_LDS_PRE 32u
#define PTX_TEXT_LDS_SRC (PTX_TEXT_LDS_PRE + ((4u * (PTX_TEXT_TILE + 1u) + 15u) & ~15u))
#define PTX_TEXT_LDS_LONG (PTX_TEXT_LDS_SRC + 8u * PTX_TEXT_TILE)
#define PTX_TEXT_LDS_BYTES (PTX_TEXT_LDS_LONG + 2u * PTX_TEXT_TILE)
static_assert(sizeof(PtxTextHdr) == PTX_TEXT_LDS_PRE, "the header fills the first 32 bytes of a wave's LDS");

/* rows of a log's `values` / `spans` that can exist: a log never produces more rows than it has ops, so a count beyond that (a result that is not this batch's
 * merge) is cut to the log's own rows and no pass reads a neighbour's */
PTX_DEV uint32_t ptx_text_rows(const PtxTextArgs& A, uint32_t log, uint32_t count) {
    const uint64_t rows = A.log_off[log + 1] - A.log_off[log];
    return (uint64_t)count < rows ? count : (uint32_t)rows;
}

typedef uint32_t __attribute__((may_alias)) ptx_text_u32;
/* two units with one dword store; p stands on an even unit of a buffer whose first unit is dword-aligned */
PTX_DEV void ptx_text_store2(uint16_t* p, uint32_t lo, uint32_t hi) { *(ptx_text_u32*)__builtin_assume_aligned(p, 4) = lo | (hi << 16); }

template <uint32_t kThreads>
PTX_DEV void ptx_text_length_log(const PtxTextArgs& A, uint32_t l, uint8_t* lds) {
    PtxTextHdr* H = (PtxTextHdr*)lds;
    const uint32_t log = A.first_log + l;
    const ptx_log_result r = A.logs[log];
    const uint32_t* vals = A.values + A.log_off[log];
    const uint32_t nv = r.status == PTX_OK ? ptx_text_rows(A, log, r.n_visible) : 0u;
    PTX_LEADER {
        H->sum = 0;
        H->bad = 0;
    }
    PTX_SYNC_T();
    unsigned long long sum = 0;
    uint32_t bad = 0;
    PTX_FOR(i, nv) {
        const uint32_t id = vals[i];
        if (id >= A.n_strings) bad |= 1u; /* checked before the table is read: never an out-of-range read */
        else {
            const uint64_t n = A.str_off[id + 1u] - A.str_off[id];
            if (n >> 32) bad |= 2u;
            else sum += n;
        }
    }
    ptx_reduce_add64(&H->sum, sum);
    if (bad) ptx_atomic_or(&H->bad, bad);
    PTX_SYNC_T();
    PTX_LEADER {
        const uint32_t st = r.status != PTX_OK ? r.status : (H->bad & 1u) ? (uint32_t)PTX_ERR_BAD_OP : ((H->bad & 2u) || (H->sum >> 32)) ? (uint32_t)PTX_ERR_CAPACITY : (uint32_t)PTX_OK;
        A.status[l] = st;
        A.off[l] = st == PTX_OK ? H->sum : 0ull;
        A.off[(uint64_t)(A.n_logs + 1u) + l] = r.status == PTX_OK ? ptx_text_rows(A, log, r.n_spans) : 0u; /* == ptx_result.span_off: a failed MERGE has no spans */
    }
}

template <uint32_t kThreads>
PTX_DEV void ptx_text_assemble_log(const PtxTextArgs& A, uint32_t l, uint8_t* lds) {
    PtxTextHdr* H = (PtxTextHdr*)lds;
    uint32_t* pre = (uint32_t*)(lds + PTX_TEXT_LDS_PRE);
    uint64_t* src = (uint64_t*)(lds + PTX_TEXT_LDS_SRC);
    uint16_t* longl = (uint16_t*)(lds + PTX_TEXT_LDS_LONG);
    const uint32_t log = A.first_log + l;
    const uint64_t* span_off = A.off + (uint64_t)(A.n_logs + 1u);
    uint32_t* su = A.span_unit + span_off[l];
    const uint32_t ns = (uint32_t)(span_off[l + 1u] - span_off[l]);
    if (A.status[l] != PTX_OK) { /* no text; the spans a good merge has (a text-only failure: BAD_OP, CAPACITY) all start at unit 0 */
        PTX_FOR(k, ns) su[k] = 0u;
        return;
    }
    const uint32_t nv = ptx_text_rows(A, log, A.logs[log].n_visible);
    const uint32_t* vals = A.values + A.log_off[log];
    const ptx_span* sp = A.spans + A.log_off[log];
    uint16_t* dst = A.text + A.off[l];
    const uint32_t total = (uint32_t)(A.off[l + 1u] - A.off[l]);
    uint32_t carry = 0; /* units before the tile */
    uint32_t sk = 0;    /* spans done */
    for (uint32_t t0 = 0; t0 < nv; t0 += PTX_TEXT_TILE) {
        const uint32_t nt = nv - t0 < PTX_TEXT_TILE ? nv - t0 : PTX_TEXT_TILE;
        PTX_LEADER {
            H->run = 0;
            H->not_one = 0;
            H->n_long = 0;
        }
        PTX_SYNC_T();
        /* ---- ids -> (offset, length), the scan ---- */
        PTX_GEN_FOR(lane, 64u) {
            const uint32_t e0 = lane * PTX_TEXT_PER_LANE;
            uint32_t ln[PTX_TEXT_PER_LANE], cnt = 0, odd = 0;
            uint64_t so[PTX_TEXT_PER_LANE];
            for (uint32_t j = 0; j < PTX_TEXT_PER_LANE; ++j) {
                ln[j] = 0;
                so[j] = 0;
                if (e0 + j < nt) {
                    const uint32_t id = vals[t0 + e0 + j]; /* < n_strings: the length pass has seen every id of a log whose status is PTX_OK */
                    so[j] = A.str_off[id];
                    ln[j] = (uint32_t)(A.str_off[id + 1u] - so[j]);
                    odd |= ln[j] != 1u;
                }
                cnt += ln[j];
            }
            uint32_t p = carry + ptx_append_n(&H->run, cnt); /* (the cursor starts every tile at 0: a tile of empty strings only gets `carry` too) */
            for (uint32_t j = 0; j < PTX_TEXT_PER_LANE; ++j) {
                if (e0 + j < nt) {
                    pre[e0 + j] = p;
                    src[e0 + j] = so[j];
                }
                p += ln[j];
            }
            if (e0 < nt && e0 + PTX_TEXT_PER_LANE >= nt) pre[nt] = p; /* the lane of the tile's last element: the tile's end */
            if (odd) ptx_atomic_or(&H->not_one, 1u);
        }
        PTX_SYNC_T();
        /* ---- the copy ---- */
        if (PTX_U32(H->not_one) == 0u) {
            PTX_FOR(lane, 64u) {
                const uint32_t e0 = lane * PTX_TEXT_PER_LANE;
                if (e0 + PTX_TEXT_PER_LANE <= nt) {
                    static_assert(PTX_TEXT_PER_LANE == 4u, "the packed stores below are written for four units per lane");
                    const uint32_t u0 = A.units[src[e0]], u1 = A.units[src[e0 + 1u]], u2 = A.units[src[e0 + 2u]], u3 = A.units[src[e0 + 3u]];
                    uint16_t* d = dst + pre[e0];
                    if (((uintptr_t)d & 2u) == 0u) {
                        ptx_text_store2(d, u0, u1);
                        ptx_text_store2(d + 2, u2, u3);
                    } else {
                        d[0] = (uint16_t)u0;
                        ptx_text_store2(d + 1, u1, u2);
                        d[3] = (uint16_t)u3;
                    }
                } else {
                    for (uint32_t e = e0; e < nt; ++e) dst[pre[e]] = A.units[src[e]];
                }
            }
        } else {
            PTX_FOR(lane, 64u) {
                for (uint32_t j = 0; j < PTX_TEXT_PER_LANE; ++j) {
                    const uint32_t e = lane * PTX_TEXT_PER_LANE + j;
                    if (e < nt) {
                        const uint32_t n = pre[e + 1u] - pre[e];
                        if (n <= PTX_TEXT_LANE_MAX) {
                            const uint16_t* s = A.units + src[e];
                            uint16_t* d = dst + pre[e];
                            for (uint32_t u = 0; u < n; ++u) d[u] = s[u];
                        } else {
                            longl[ptx_append(&H->n_long, true)] = (uint16_t)e;
                        }
                    }
                }
            }
            PTX_SYNC_T();
            const uint32_t nl = PTX_U32(H->n_long);
            for (uint32_t k = 0; k < nl; ++k) {
                const uint32_t e = longl[k], n = pre[e + 1u] - pre[e];
                const uint16_t* s = A.units + src[e];
                uint16_t* d = dst + pre[e];
                PTX_FOR(u, n) d[u] = s[u];
            }
        }
        /* ---- the spans whose first element stands in this tile, 64 per step ---- */
        for (;;) {
            PTX_BALLOT64(here, q0, (sk + q0 < ns && sp[sk + q0].start < t0 + nt))
            PTX_FOR(q, 64u) {
                if ((here >> q) & 1ull) {
                    const uint32_t st = sp[sk + q].start;
                    su[sk + q] = pre[st >= t0 ? st - t0 : 0u];
                }
            }
            const uint32_t c = (uint32_t)__builtin_popcountll(here);
            sk += c;
            if (c < 64u) break;
        }
        carry = PTX_U32(pre[nt]);
        PTX_SYNC_T(); /* the next tile rewrites the LDS */
    }
    PTX_FOR(k, ns - sk) su[sk + k] = total; /* (spans that start behind the last element do not exist in a merge's result) */
}
