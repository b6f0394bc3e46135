/*
 * find_core.h — a pattern searched in the text of resident documents, the hits as ranges of visible ELEMENT indexes (ptx_result_find_text).
 *
 * The reference has no search: its documents are JS strings and a caller writes text.indexOf(pattern, from) in a loop over the text getTextWithFormatting
 * returns (reference/src/peritext.ts:337-395).  What is pinned here is String.prototype.indexOf repeated from p + 1: every position p with
 * text[p + i] == pattern[i] for all i < m, overlapping ones included, compared over UTF-16 CODE UNITS.  A hit is reported as the unit offset within the log's
 * text and as [hit_start, hit_end): the visible indexes of the elements that hold its first and its last unit, the end exclusive — what delete {index, count},
 * addMark {startIndex, endIndex} (peritext.ts:491-497) and a cursor request take.
 *
 * The text is the one text_core.h assembles (lengths, offsets, assemble: unchanged), into a pool block that never leaves the device.  Then, ONE 64-lane wave
 * per log for the reason text_core.h gives (the logs fill the machine, not the lanes of one log):
 *
 *   ptx_find_count_log  walks the log's candidate positions 0 .. L - m in steps of PTX_FIND_STEP = 64 lanes x PTX_FIND_PER_LANE.  A step stages its units and a
 *                       halo of m - 1 more into LDS — the halo ends where the LOG ends, never in the next log's text, which lies directly behind it — folded
 *                       ('A'..'Z' -> 'a'..'z') when PTX_FIND_ASCII_NOCASE is set; the pattern lies in LDS too, folded once.  Position slot j of lane q is
 *                       j * 64 + q: a ballot per slot has the hits of 64 CONSECUTIVE positions in its bits, the count is a popcount in a scalar register —
 *                       no reduction, no atomic.  A log starts at whatever parity the one before ended on: units are loaded one by one, consecutive lanes on
 *                       consecutive units.  L < m is zero steps.
 *   (the host library scans min(n_matches, cap) into hit_off: ptx_find_offsets_kernel, the twin of ptx_text_offsets_kernel)
 *   ptx_find_emit_log   the same walk again; a hit's slot in the log's list is the hits before the step + the popcount of the ballot bits below its lane:
 *                       ascending by construction, and the walk stops at the cap.  Then the elements: tiles of PTX_TEXT_TILE with the length scan of the
 *                       assemble pass; two forward cursors over the log's listed hits — the first unit's and the last unit's — resolve through the tile's
 *                       scan in LDS: the holder of unit u is the LAST element of the tile with pre[e] <= u (a binary search; an empty string before the
 *                       holder has pre[e] == pre[holder] and is passed over, one behind it has pre[e] > u).  A hit whose two units lie in different tiles
 *                       is why there are two cursors.  The walk ends with the last listed hit, not with the log.
 *
 * Plain vector loads and stores only; written against the platform layer like the other cores: hipcc builds it into the product, tests/emu/emu_find.cc plays it
 * on one host thread.
 */
#pragma once
#include "text_core.h"

#define PTX_FIND_PER_LANE 4u                          /* position slots of a lane */
#define PTX_FIND_STEP (64u * PTX_FIND_PER_LANE)       /* candidate positions per step of the walk (mirrored in peritext_amd/abi.py: the tests take their edge sizes from it) */
/* (PTX_FIND_PATTERN_MAX, the longest pattern in code units, and PTX_FIND_ASCII_NOCASE are the C ABI's: include/peritext_hip.h) */

struct PtxFindArgs {
    PtxTextArgs T;             /* the text passes' arguments: status, off (text_off | span_off), text, and what the element walk reads (log_off, logs, values, str_off) */
    const uint16_t* pattern;   /* device [n_pattern] */
    uint32_t n_pattern, flags;
    uint32_t cap, pad;         /* max_hits_per_log */
    uint32_t* n_matches;       /* [n_logs] */
    uint64_t* hit_off;         /* [n_logs + 1] */
    uint32_t* hit_unit;        /* [hit_off[n_logs]] */
    uint32_t* hit_start;
    uint32_t* hit_end;
};

struct PtxFindHdr {
    uint32_t run; /* emit: cursor of the tile's scan */
    uint32_t pad[7];
};
/* LDS of a wave: header | the pattern | the step's units and their halo | unit offset of every element of the tile, and the tile's end */
#define PTX_FIND_LDS_PAT 32u
#define PTX_FIND_LDS_WIN (PTX_FIND_LDS_PAT + 2u * PTX_FIND_PATTERN_MAX)
#define PTX_FIND_LDS_PRE (PTX_FIND_LDS_WIN + ((2u * (PTX_FIND_STEP + PTX_FIND_PATTERN_MAX - 1u) + 15u) & ~15u))
#define PTX_FIND_LDS_BYTES (PTX_FIND_LDS_PRE + ((4u * (PTX_TEXT_TILE + 1u) + 15u) & ~15u))
static_assert(sizeof(PtxFindHdr) == PTX_FIND_LDS_PAT, "the header fills the first 32 bytes of a wave's LDS");

PTX_DEV uint32_t ptx_find_fold(uint32_t u, bool nocase) { return nocase && u - 0x41u < 26u ? u + 0x20u : u; } /* no other unit is folded: U+0130, U+212A stay */

PTX_DEV bool ptx_find_match(const uint16_t* w, const uint16_t* pat, uint32_t m) {
    for (uint32_t i = 0; i < m; ++i)
        if (w[i] != pat[i]) return false;
    return true;
}

/* The walk of both passes: the number of matches of log l — kEmit: of those up to and including the step in which the nh-th was listed, hu[0 .. nh) written. */
template <uint32_t kThreads, bool kEmit>
PTX_DEV uint32_t ptx_find_walk(const PtxFindArgs& A, uint32_t l, uint8_t* lds, uint32_t nh, uint32_t* hu) {
    uint16_t* pat = (uint16_t*)(lds + PTX_FIND_LDS_PAT);
    uint16_t* win = (uint16_t*)(lds + PTX_FIND_LDS_WIN);
    const uint32_t m = A.n_pattern;
    const uint64_t at = A.T.off[l];
    const uint32_t L = (uint32_t)(A.T.off[l + 1u] - at); /* < 2^32: the length pass made a longer text PTX_ERR_CAPACITY */
    if (A.T.status[l] != PTX_OK || L < m) return 0u;
    const uint16_t* txt = A.T.text + at;
    const bool nocase = (A.flags & PTX_FIND_ASCII_NOCASE) != 0u;
    PTX_FOR(i, m) pat[i] = (uint16_t)ptx_find_fold(A.pattern[i], nocase);
    const uint32_t P = L - m + 1u; /* candidate positions: none beyond L - m */
    uint32_t found = 0;
    for (uint32_t s0 = 0;; s0 += PTX_FIND_STEP) {
        const uint32_t np = P - s0 < PTX_FIND_STEP ? P - s0 : PTX_FIND_STEP; /* positions of the step */
        const uint32_t nu = np + m - 1u;                                     /* its units and the halo: s0 + nu <= L, the halo ends with the LOG */
        PTX_SYNC_T(); /* the pattern is written; the step before has been read */
        PTX_FOR(i, nu) win[i] = (uint16_t)ptx_find_fold(txt[s0 + i], nocase);
        PTX_SYNC_T();
        for (uint32_t j0 = 0; j0 < np; j0 += 64u) {
            PTX_BALLOT64(hit, q0, (j0 + q0 < np && ptx_find_match(win + j0 + q0, pat, m)))
            if (kEmit) {
                PTX_FOR(q, 64u) {
                    const uint32_t slot = found + (uint32_t)__builtin_popcountll(hit & ((1ull << q) - 1ull));
                    if (((hit >> q) & 1ull) && slot < nh) hu[slot] = s0 + j0 + q;
                }
            }
            found += (uint32_t)__builtin_popcountll(hit);
            if (kEmit && found >= nh) return found; /* the cap: the listed hits are the FIRST nh */
        }
        if (P - s0 <= PTX_FIND_STEP) break; /* (s0 never passes P: no wrap at texts of nearly 2^32 units) */
    }
    return found;
}

template <uint32_t kThreads>
PTX_DEV void ptx_find_count_log(const PtxFindArgs& A, uint32_t l, uint8_t* lds) {
    const uint32_t n = ptx_find_walk<kThreads, false>(A, l, lds, 0u, nullptr);
    PTX_LEADER A.n_matches[l] = n;
}

/* the element of the tile that holds unit u: the last e < nt with pre[e] <= u.  pre[0] <= u < pre[nt] (the caller's cursors see to both) */
PTX_DEV uint32_t ptx_find_holder(const uint32_t* pre, uint32_t nt, uint32_t u) {
    uint32_t lo = 0, hi = nt;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* The position half of the emit pass, callable alone (view_core.h maps the hits to elements by a search over a resident prefix instead of the tile walk below):
 * hit_unit of the log's listed hits — the first hit_off[l + 1] - hit_off[l] of them.  Returns their number: 0 for a log without text, without a match, or in a
 * count-only call.  Reads nothing of T but status, off and text. */
template <uint32_t kThreads>
PTX_DEV uint32_t ptx_find_positions_log(const PtxFindArgs& A, uint32_t l, uint8_t* lds) {
    const uint32_t nh = (uint32_t)(A.hit_off[l + 1u] - A.hit_off[l]);
    if (nh != 0u) (void)ptx_find_walk<kThreads, true>(A, l, lds, nh, A.hit_unit + A.hit_off[l]);
    return nh;
}

template <uint32_t kThreads>
PTX_DEV void ptx_find_emit_log(const PtxFindArgs& A, uint32_t l, uint8_t* lds) {
    PtxFindHdr* H = (PtxFindHdr*)lds;
    uint32_t* pre = (uint32_t*)(lds + PTX_FIND_LDS_PRE);
    const uint32_t nh = ptx_find_positions_log<kThreads>(A, l, lds);
    if (nh == 0u) return;
    const uint32_t* hu = A.hit_unit + A.hit_off[l];
    uint32_t* hs = A.hit_start + A.hit_off[l];
    uint32_t* he = A.hit_end + A.hit_off[l];
    PTX_SYNC_FULL(); /* a lane's hit_unit stores are read by other lanes below */
    const uint32_t log = A.T.first_log + l;
    const uint32_t nv = ptx_text_rows(A.T, log, A.T.logs[log].n_visible);
    const uint32_t* vals = A.T.values + A.T.log_off[log];
    const uint32_t last = A.n_pattern - 1u;
    uint32_t carry = 0;      /* units before the tile */
    uint32_t ks = 0, ke = 0; /* hits whose first / last unit has its element */
    for (uint32_t t0 = 0; t0 < nv && ke < nh; t0 += PTX_TEXT_TILE) { /* (ks >= ke: a hit's first unit stands no later than its last) */
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
                if (e0 + j < nt) pre[e0 + j] = p;
                p += ln[j];
            }
            if (e0 < nt && e0 + PTX_TEXT_PER_LANE >= nt) pre[nt] = p; /* the lane of the tile's last element: the tile's end */
        }
        PTX_SYNC_T();
        const uint32_t end = PTX_U32(pre[nt]);
        /* the hits whose first unit stands in this tile, 64 per step; then those whose last unit does */
        for (;;) {
            PTX_BALLOT64(here, q0, (ks + q0 < nh && hu[ks + q0] < end))
            PTX_FOR(q, 64u) {
                if ((here >> q) & 1ull) hs[ks + q] = t0 + ptx_find_holder(pre, nt, hu[ks + q]);
            }
            const uint32_t c = (uint32_t)__builtin_popcountll(here);
            ks += c;
            if (c < 64u) break;
        }
        for (;;) {
            PTX_BALLOT64(here, q0, (ke + q0 < nh && hu[ke + q0] + last < end))
            PTX_FOR(q, 64u) {
                if ((here >> q) & 1ull) he[ke + q] = t0 + ptx_find_holder(pre, nt, hu[ke + q] + last) + 1u;
            }
            const uint32_t c = (uint32_t)__builtin_popcountll(here);
            ke += c;
            if (c < 64u) break;
        }
        carry = end;
        PTX_SYNC_T(); /* the next tile rewrites the LDS */
    }
    /* (every unit of the text stands in an element: nothing is left — a result that is not this batch's merge gets the log's end, not stale memory) */
    PTX_FOR(k, nh - ks) hs[ks + k] = nv;
    PTX_FOR(k, nh - ke) he[ke + k] = nv;
}
