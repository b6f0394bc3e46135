/*
 * replay_hbm_core.h — the patch stream of a replica log whose replay state does not fit one CU's LDS (beside replay_core.h as biglog_core.h sits beside
 * merge_core.h).
 *
 * The same algorithm, the same records in the same order as ptx_replay_log<T, true, true> (32-bit ranks and slots) — what changes is where the state lives: every
 * array whose size grows with the document (n, K, Kc, Kid) is in a slice of global scratch sized by ptx_replay_hbm_units_hdr, read and written with the
 * workgroup-scope accessors (ptx_coherent_*) and a wait for the wave's outstanding stores (ptx_global_stores_done) at the head of every op and wherever a lane
 * reads, within one op, what another lane has just written.  The LDS holds what does not grow: the header, the 32-row chunk buffers, ONE TILE of the per-word
 * cw / cnt of a mark op (PTX_HBM_TILE words; a longer range is worked through tile by tile, the record count carried across), and the top levels of the two
 * summaries below (bounded by n <= 0x03FFFFFF).  One 64-thread workgroup (one wave) per log, as replay_core.h.
 *
 * Three loops of replay_core.h walk the whole state per op and would be quadratic in HBM; here they are:
 *   visible index (present[w].pre +- 1 for every word above the rank)
 *       -> THREE levels of prefixes: present[w].pre counts from the start of the word's BLOCK of 64 words, bpre[b] from the start of the block's SUPERBLOCK of
 *          64 blocks (both in HBM), spre[s] from the start of the document (LDS, at most 513 entries).  rank = spre + bpre + pre + popcount of the bits below:
 *          three independent loads, by any lane.  An insert / delete rewrites one word, the at most 63 prefixes behind it in its block (one load and one store
 *          per lane), the at most 63 behind its block in the superblock, and the LDS entries.
 *   closest defined slot to the left (ptx_last_set_below: 64 words per step from the top down)
 *       -> a summary per level, "word i of the level below is non-zero": d1 over defined, d2 over d1 (HBM), d3 over d2 (LDS, at most 129 words).  The search
 *          climbs while the masked word of a level is empty and descends through the highest bit: at most six dependent loads, one when the word that holds
 *          the slot has a defined one below it; none at all while nothing is defined (a counter in a register).
 *   next defined slot of the range (PTX_NEXT_AFTER_WORD: word by word upwards)
 *       -> the same summaries, searched upwards.
 *
 * Compiled two ways like the other kernel sources (hipcc: ptx_replay_kernel_hbm; g++ -DPTX_EMU: tests/emu/emu_replay_hbm.cc).
 */
#pragma once
#include "replay_core.h"

#define PTX_HBM_TILE 1024u    /* words (of 32 boundary slots) of a mark op's range worked through at a time: 8 KB of LDS for cw / cnt */
#define PTX_HBM_SUP_MAX 516u  /* superblocks of 64 x 64 words of `present` a log of 0x03FFFFFF elements has (513), rounded up */
#define PTX_HBM_D3_MAX 132u   /* words of the top summary of `defined` such a log has (129), rounded up */
#define PTX_REPLAY_HBM_LDS_BYTES 12288u /* header + spre + d3 + chunk buffers + one tile of cw / cnt (11 744), rounded up */
#define PTX_HBM_NONE 0xFFFFFFFFu

struct PtxReplayHbmArgs {
    PtxReplayArgs R;           /* (win_scratch / win_off / lds_bytes are not read) */
    uint32_t* state;           /* the replay state of every log of log_index ... */
    const uint64_t* state_off; /* ... [n_hbm + 1], in u32 units: the slice of the k-th of them (ptx_replay_hbm_units_hdr of its header); the kernel zeroes what it needs zeroed */
    const uint32_t* log_index; /* [n_hbm]: the logs this launch replays */
    uint32_t n_hbm;
};

/* where the arrays of a log's slice start (u32 units, every array 16-byte aligned).  [present, zero_end) must read zero when the replay starts. */
struct PtxHbmLayout {
    uint64_t present, bpre, d0, d1, d2, mb, cadd, zero_end, lurl, tab, ca, cb, cprev, ccid, ctail, end;
    uint32_t nwe, nblk, nsup, nw0, nw1, nw2, nw3;
};
PTX_HD uint64_t ptx_hbm_a4(uint64_t units) { return (units + 3u) & ~3ull; }
PTX_HD PtxHbmLayout ptx_replay_hbm_layout(uint64_t n, uint64_t K, uint64_t Kc, uint64_t Kid) {
    PtxHbmLayout L;
    const uint64_t nwe = (n >> 5) + 2, nws = ((2 * n + 2) >> 5) + 2, Kl = K - Kc;
    L.nwe = (uint32_t)nwe;
    L.nblk = (uint32_t)((nwe + 63) >> 6);
    L.nsup = (L.nblk + 63u) >> 6;
    L.nw0 = (uint32_t)nws;
    L.nw1 = (L.nw0 + 31u) >> 5;
    L.nw2 = (L.nw1 + 31u) >> 5;
    L.nw3 = (L.nw2 + 31u) >> 5;
    uint64_t o = 0;
    L.present = o, o += ptx_hbm_a4(2 * nwe);        /* PtxBitWord {bits, prefix inside the block of 64 words} */
    L.bpre = o, o += ptx_hbm_a4(L.nblk);            /* prefix of the block inside its superblock of 64 blocks */
    L.d0 = o, o += ptx_hbm_a4(nws);                 /* `defined`: bit per boundary slot */
    L.d1 = o, o += ptx_hbm_a4(L.nw1);               /* bit per word of d0: non-zero */
    L.d2 = o, o += ptx_hbm_a4(L.nw2);               /* bit per word of d1: non-zero */
    L.mb = o, o += ptx_hbm_a4(4 * nws);             /* PtxMarkBits per word of slots */
    L.cadd = o, o += ptx_hbm_a4((Kc >> 5) + 1);     /* bit per comment op: it is an addMark */
    L.zero_end = o;
    L.lurl = o, o += ptx_hbm_a4(2 * n + 2);         /* per slot: the url of the winning link */
    L.tab = o, o += ptx_hbm_a4(4 * (Kl + 1));       /* applied LWW mark op: {row | start slot << 32, end of its interval} */
    L.ca = o, o += ptx_hbm_a4(Kc + 1);              /* comment op: first covered slot ... */
    L.cb = o, o += ptx_hbm_a4(Kc + 1);              /* ... first slot not covered */
    L.cprev = o, o += ptx_hbm_a4((Kc + 2) >> 1);    /* u16: chain of the ops with the same id */
    L.ccid = o, o += ptx_hbm_a4((Kc + 2) >> 1);     /* u16: comment op: its id */
    L.ctail = o, o += ptx_hbm_a4((Kid + 2) >> 1);   /* u16: per comment id: the last registered op */
    L.end = o;
    return L;
}
/* u32 units of state scratch a log takes */
PTX_HD uint64_t ptx_replay_hbm_units(uint64_t n, uint64_t K, uint64_t Kc, uint64_t Kid) { return ptx_replay_hbm_layout(n, K, Kc, Kid).end; }
PTX_HD uint64_t ptx_replay_hbm_units_hdr(const ptx_log_hdr& h) {
    const uint64_t K = (uint64_t)h.n_mark[0] + h.n_mark[1] + h.n_mark[2] + h.n_mark[3];
    return ptx_replay_hbm_units(h.n_ins, K, h.n_mark[PTX_MARK_COMMENT], h.n_mark[PTX_MARK_COMMENT] ? h.n_comment_ids : 0u);
}

/* the state of one log: pointers into its slice (and, for spre / d3, the LDS) */
struct PtxHbmState {
    PtxBitWord* present;
    uint32_t *bpre, *spre;
    uint32_t *d0, *d1, *d2, *d3;
    uint32_t nwe, nblk, nsup, nw0, nw1, nw2, nw3;
    PtxMarkBits* mb;
    uint32_t* lurl;
};

/* # visible elements strictly below rank `pos` (any lane, any pos <= n + 31) */
PTX_DEV uint32_t ptx_hbm_rank(const PtxHbmState& S, uint32_t pos) {
    const uint32_t w = pos >> 5;
    const uint32_t bits = ptx_coherent_load32(&S.present[w].bits), pre = ptx_coherent_load32(&S.present[w].pre), bp = ptx_coherent_load32(&S.bpre[w >> 6]);
    return S.spre[w >> 12] + bp + pre + ptx_popc(bits & ((1u << (pos & 31u)) - 1u));
}
PTX_DEV uint32_t ptx_hbm_top_bit(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }
/* position + 1 of the highest defined slot strictly below `lim`, 0 when there is none (any lane) */
PTX_DEV uint32_t ptx_hbm_last_below(const PtxHbmState& S, uint32_t lim) {
    if (lim == 0u) return 0u;
    uint32_t w = (lim - 1u) >> 5, m = ptx_coherent_load32(&S.d0[w]) & ptx_bits_below(((lim - 1u) & 31u) + 1u);
    if (m) return (w << 5) + ptx_hbm_top_bit(m) + 1u;
    if (w == 0u) return 0u; /* (from here on: the highest non-zero word of a level strictly below index w) */
    uint32_t lev = 1u, hit;
    m = ptx_coherent_load32(&S.d1[(w - 1u) >> 5]) & ptx_bits_below(((w - 1u) & 31u) + 1u);
    if (!m) {
        w = (w - 1u) >> 5;
        if (w == 0u) return 0u;
        lev = 2u;
        m = ptx_coherent_load32(&S.d2[(w - 1u) >> 5]) & ptx_bits_below(((w - 1u) & 31u) + 1u);
        if (!m) {
            w = (w - 1u) >> 5;
            if (w == 0u) return 0u;
            lev = 3u;
            uint32_t v = (w - 1u) >> 5;
            m = S.d3[v] & ptx_bits_below(((w - 1u) & 31u) + 1u);
            while (!m && v) m = S.d3[--v];
            if (!m) return 0u;
            w = (v << 5) + 1u; /* (so that (w - 1) >> 5 below names word v) */
        }
    }
    hit = (((w - 1u) >> 5) << 5) + ptx_hbm_top_bit(m);
    if (lev >= 3u) hit = (hit << 5) + ptx_hbm_top_bit(ptx_coherent_load32(&S.d2[hit]));
    if (lev >= 2u) hit = (hit << 5) + ptx_hbm_top_bit(ptx_coherent_load32(&S.d1[hit]));
    hit = (hit << 5) + ptx_hbm_top_bit(ptx_coherent_load32(&S.d0[hit]));
    return hit + 1u;
}
/* the lowest defined slot at or above `pos`, PTX_HBM_NONE when there is none (any lane) */
PTX_DEV uint32_t ptx_hbm_first_from(const PtxHbmState& S, uint32_t pos) {
    uint32_t w = pos >> 5;
    if (w >= S.nw0) return PTX_HBM_NONE;
    uint32_t m = ptx_coherent_load32(&S.d0[w]) & ptx_bits_from(pos & 31u);
    if (m) return (w << 5) + (uint32_t)__builtin_ctz(m);
    uint32_t lev = 1u, p = w + 1u, hit; /* (from here on: the lowest non-zero word of a level at or above index p) */
    if ((p >> 5) >= S.nw1) return PTX_HBM_NONE;
    m = ptx_coherent_load32(&S.d1[p >> 5]) & ptx_bits_from(p & 31u);
    if (!m) {
        p = (p >> 5) + 1u;
        if ((p >> 5) >= S.nw2) return PTX_HBM_NONE;
        lev = 2u;
        m = ptx_coherent_load32(&S.d2[p >> 5]) & ptx_bits_from(p & 31u);
        if (!m) {
            p = (p >> 5) + 1u;
            uint32_t v = p >> 5;
            if (v >= S.nw3) return PTX_HBM_NONE;
            lev = 3u;
            m = S.d3[v] & ptx_bits_from(p & 31u);
            while (!m && ++v < S.nw3) m = S.d3[v];
            if (!m) return PTX_HBM_NONE;
            p = v << 5;
        }
    }
    hit = ((p >> 5) << 5) + (uint32_t)__builtin_ctz(m);
    if (lev >= 3u) hit = (hit << 5) + (uint32_t)__builtin_ctz(ptx_coherent_load32(&S.d2[hit]));
    if (lev >= 2u) hit = (hit << 5) + (uint32_t)__builtin_ctz(ptx_coherent_load32(&S.d1[hit]));
    return (hit << 5) + (uint32_t)__builtin_ctz(ptx_coherent_load32(&S.d0[hit]));
}
/* ONE lane: slot s becomes a defined one (the summaries follow where its word was empty) */
PTX_DEV void ptx_hbm_set_defined(const PtxHbmState& S, uint32_t s) {
    uint32_t i = s >> 5;
    uint32_t old = ptx_coherent_load32(&S.d0[i]);
    ptx_coherent_store32(&S.d0[i], old | (1u << (s & 31u)));
    if (old) return;
    old = ptx_coherent_load32(&S.d1[i >> 5]);
    ptx_coherent_store32(&S.d1[i >> 5], old | (1u << (i & 31u)));
    if (old) return;
    i >>= 5;
    old = ptx_coherent_load32(&S.d2[i >> 5]);
    ptx_coherent_store32(&S.d2[i >> 5], old | (1u << (i & 31u)));
    if (old) return;
    i >>= 5;
    S.d3[i >> 5] |= 1u << (i & 31u);
}
/* every lane: the element of rank r becomes visible (d = 1) or stops being so (d = -1): its bit, and the prefixes behind it on the three levels */
template <uint32_t kThreads>
PTX_DEV void ptx_hbm_present_flip(const PtxHbmState& S, uint32_t r, uint32_t d) {
    const uint32_t w = r >> 5, blk = w >> 6, sup = blk >> 6;
    PTX_FOR(j, 64u) {
        const uint32_t ww = (blk << 6) + j;
        if (ww == w) ptx_coherent_store32(&S.present[ww].bits, ptx_coherent_load32(&S.present[ww].bits) ^ (1u << (r & 31u)));
        else if (ww > w && ww < S.nwe) ptx_coherent_store32(&S.present[ww].pre, ptx_coherent_load32(&S.present[ww].pre) + d);
    }
    PTX_FOR(j, 64u) {
        const uint32_t bb = (sup << 6) + j;
        if (bb > blk && bb < S.nblk) ptx_coherent_store32(&S.bpre[bb], ptx_coherent_load32(&S.bpre[bb]) + d);
    }
    PTX_FOR(s, S.nsup) {
        if (s > sup) S.spre[s] += d;
    }
}
PTX_DEV void ptx_hbm_fail(const PtxReplayArgs& A, uint32_t log, uint32_t status) {
    ptx_patch_log pl;
    pl.status = status;
    pl.n_patches = 0;
    A.plogs[log] = pl;
    if (A.ext_off) A.ext_off[3 * (uint64_t)log] = A.ext_off[3 * (uint64_t)log + 1] = ~0ull;
}

template <uint32_t kThreads>
PTX_DEV void ptx_replay_log_hbm(const PtxReplayHbmArgs& HA, uint32_t k, uint8_t* lds) {
    typedef PtxChunkRowT<true> PtxChunkRow;
    const PtxReplayArgs& A = HA.R;
    const uint32_t log = HA.log_index[k];
    const uint32_t SLOT_NONE = 0xFFFFFFFFu;
    PtxReplayHdr* H = (PtxReplayHdr*)lds;
    const uint64_t base = A.log_off[log];
    const uint32_t N = (uint32_t)(A.log_off[log + 1] - base);
    PtxPatchDst dst;
    dst.out = A.patches + A.patch_off[log];
    dst.pcap = (uint32_t)(A.patch_off[log + 1] - A.patch_off[log]);
    dst.H = H;
    dst.patches = A.patches;
    uint32_t room = dst.pcap;                   /* records the log can hold: its capacity + its extents */
    uint32_t ext_left = A.arena_next ? 2u : 0u; /* extents it may still ask for */
    const uint32_t first = A.first_row ? A.first_row[log] : 0u;
    const uint64_t* op_id = A.op_id + base;
    const uint32_t* payload = A.payload + base;
    const uint8_t* action = A.action + base;
    const uint8_t* mark_type = A.mark_type + base;
    const uint32_t* erank = A.elem_rank + base;
    const uint32_t* refs = A.refs + base;

    const uint32_t merge_status = A.res[log].status;
    if (merge_status != PTX_OK || N == 0) { /* the reference threw somewhere in this log: no stream (the status says why) */
        PTX_LEADER { ptx_hbm_fail(A, log, merge_status); }
        return;
    }
    const ptx_log_hdr hd = A.log_hdr[log];
    const uint32_t n = hd.n_ins, Kc = hd.n_mark[PTX_MARK_COMMENT];
    const uint32_t Kid = Kc ? hd.n_comment_ids : 0u;
    const uint32_t K = hd.n_mark[0] + hd.n_mark[1] + hd.n_mark[2] + hd.n_mark[3];
    const uint32_t Kl = K - Kc;
    const uint32_t toff[3] = {0u, hd.n_mark[PTX_MARK_STRONG], hd.n_mark[PTX_MARK_STRONG] + hd.n_mark[PTX_MARK_EM]};
    const PtxHbmLayout Lo = ptx_replay_hbm_layout(n, K, Kc, Kid);
    /* the bounds of the wide build (comment-op indices and ids stay 16 bits wide); a result without the slots' high halves cannot say where the marks of a log of
     * more than 32 766 elements are; a slice that is too small (never from this library's host) is refused, not overrun */
    if (n > 0x03FFFFFFu || Kc > 65534u || Kid > 65535u || (n > 32766u && !A.refs_hi) || HA.state_off[k + 1] - HA.state_off[k] < Lo.end || Lo.nsup > PTX_HBM_SUP_MAX ||
        Lo.nw3 > PTX_HBM_D3_MAX) {
        PTX_LEADER { ptx_hbm_fail(A, log, PTX_ERR_CAPACITY); }
        return;
    }
    uint32_t* g = HA.state + HA.state_off[k];
    PtxHbmState S;
    S.present = (PtxBitWord*)(g + Lo.present);
    S.bpre = g + Lo.bpre;
    S.d0 = g + Lo.d0;
    S.d1 = g + Lo.d1;
    S.d2 = g + Lo.d2;
    S.nwe = Lo.nwe, S.nblk = Lo.nblk, S.nsup = Lo.nsup, S.nw0 = Lo.nw0, S.nw1 = Lo.nw1, S.nw2 = Lo.nw2, S.nw3 = Lo.nw3;
    S.mb = (PtxMarkBits*)(g + Lo.mb);
    S.lurl = g + Lo.lurl;
    uint32_t* cadd = g + Lo.cadd;
    uint64_t* tab = (uint64_t*)(g + Lo.tab);
    uint32_t* ca = g + Lo.ca;
    uint32_t* cb = g + Lo.cb;
    uint16_t* cprev = (uint16_t*)(g + Lo.cprev);
    uint16_t* ccid = (uint16_t*)(g + Lo.ccid);
    uint16_t* ctail = (uint16_t*)(g + Lo.ctail);

    PtxBump bp;
    bp.base = lds;
    bp.off = (uint32_t)ptx_a16(sizeof(PtxReplayHdr));
    bp.cap = PTX_REPLAY_HBM_LDS_BYTES;
    bp.high = bp.off;
    bp.overflow = false;
    S.spre = ptx_alloc<uint32_t>(bp, PTX_HBM_SUP_MAX);
    S.d3 = ptx_alloc<uint32_t>(bp, PTX_HBM_D3_MAX);
    PtxChunkRow* c_row = ptx_alloc<PtxChunkRow>(bp, PTX_RCHUNK);
    uint8_t* c_kind = ptx_alloc<uint8_t>(bp, PTX_RCHUNK);
    uint32_t* cw = ptx_alloc<uint32_t>(bp, PTX_HBM_TILE);  /* one tile of a mark op's range: the changed slots -> the slots that open a record ... */
    uint32_t* cnt = ptx_alloc<uint32_t>(bp, PTX_HBM_TILE); /* ... their count -> its prefix */
    if (bp.overflow) {
        PTX_LEADER { ptx_hbm_fail(A, log, PTX_ERR_CAPACITY); }
        return;
    }
#define PTX_H_FENCE() ptx_global_stores_done()
#define PTX_H_BIT(p_, i_) ((ptx_coherent_load32(&(p_)[(i_) >> 5]) >> ((i_)&31u)) & 1u)

    /* ---- set-up: the slice is not zeroed by the host ---- */
    PTX_FOR(i, (uint32_t)(Lo.zero_end - Lo.present)) ptx_coherent_store32(&g[Lo.present + i], 0u);
    PTX_FOR(c, Kid + 1) ptx_coherent_store16(&ctail[c], PTX_CHAIN_NONE);
    PTX_FOR(i, PTX_HBM_SUP_MAX) S.spre[i] = 0u;
    PTX_FOR(i, PTX_HBM_D3_MAX) S.d3[i] = 0u;
    PTX_LEADER {
        H->tmp = 0;
        H->ext_cap[0] = H->ext_cap[1] = 0;
    }
    PTX_H_FENCE();
    PTX_SYNC_T();
    /* the wave's own counters: the same value in every lane */
    uint32_t npatch = 0, ncom = 0, ndef = 0;
    uint32_t ntab[3] = {0u, 0u, 0u};
    uint64_t maxop[3] = {0ull, 0ull, 0ull}; /* largest opId applied so far per LWW type */

#define PTX_VIS_AT(s_) ptx_hbm_rank(S, ((uint32_t)(s_) + 1u) >> 1) /* visible index at a boundary slot */
    /* make slot s_ a defined one: its state is that of the closest defined slot to the left (peritext.ts:176) */
#define PTX_DEFINE_SLOT(s_)                                                                                   \
    do {                                                                                                      \
        if (!PTX_U32(PTX_H_BIT(S.d0, (s_)))) {                                                                \
            const uint32_t l1_ = ndef ? PTX_U32(ptx_hbm_last_below(S, (s_))) : 0u; /* slot + 1 */             \
            PTX_LEADER {                                                                                      \
                const uint32_t bit_ = 1u << ((s_)&31u), ws_ = (s_) >> 5;                                      \
                if (l1_) {                                                                                    \
                    const uint32_t l_ = l1_ - 1u, lb_ = l_ & 31u, lw_ = l_ >> 5;                              \
                    const uint32_t sac_ = ptx_coherent_load32(&S.mb[lw_].ac), s0_ = ptx_coherent_load32(&S.mb[lw_].on[0]);     \
                    const uint32_t s1_ = ptx_coherent_load32(&S.mb[lw_].on[1]), s2_ = ptx_coherent_load32(&S.mb[lw_].on[2]);   \
                    if ((sac_ >> lb_) & 1u) ptx_coherent_store32(&S.mb[ws_].ac, (lw_ == ws_ ? sac_ : ptx_coherent_load32(&S.mb[ws_].ac)) | bit_);          \
                    if ((s0_ >> lb_) & 1u) ptx_coherent_store32(&S.mb[ws_].on[0], (lw_ == ws_ ? s0_ : ptx_coherent_load32(&S.mb[ws_].on[0])) | bit_);      \
                    if ((s1_ >> lb_) & 1u) ptx_coherent_store32(&S.mb[ws_].on[1], (lw_ == ws_ ? s1_ : ptx_coherent_load32(&S.mb[ws_].on[1])) | bit_);      \
                    if ((s2_ >> lb_) & 1u) {                                                                  \
                        ptx_coherent_store32(&S.mb[ws_].on[2], (lw_ == ws_ ? s2_ : ptx_coherent_load32(&S.mb[ws_].on[2])) | bit_);                         \
                        ptx_coherent_store32(&S.lurl[s_], ptx_coherent_load32(&S.lurl[l_]));                  \
                    }                                                                                         \
                }                                                                                             \
                ptx_hbm_set_defined(S, (s_));                                                                 \
            }                                                                                                 \
            ndef += 1u;                                                                                       \
            PTX_H_FENCE(); /* the next search, the passes of the op read what this lane stored */             \
            PTX_SYNC_T();                                                                                     \
        }                                                                                                     \
    } while (0)

    /* ---- the replay: PTX_RCHUNK rows are resolved in parallel, then applied one at a time ---- */
#pragma nounroll
    for (uint32_t t0 = 0; t0 < N; t0 += PTX_RCHUNK) {
    const uint32_t chunk_n = N - t0 < PTX_RCHUNK ? N - t0 : PTX_RCHUNK;
    { /* room for the records, looked after once per chunk of rows: replay_core.h's PTX_RESERVE */
        uint32_t rate = 3u * (npatch / (t0 > first ? t0 - first + 1u : 1u) + 1u);
        rate = rate < 8u ? 8u : rate;
        if (ext_left && t0 + PTX_RCHUNK > first && npatch + rate * PTX_RCHUNK > room) {
            rate *= ext_left == 2u ? 1u : 16u;
            const uint64_t want64 = (uint64_t)rate * (N - t0) + 1024u;
            const uint32_t want = want64 < 0x7FFFFFFFull - room ? (uint32_t)want64 : 0x7FFFFFFFu - room;
            PTX_LEADER {
                const unsigned long long at = ptx_atomic_add64(A.arena_next, (unsigned long long)want);
                const bool ok = at + want <= A.arena_cap;
                H->ext_ok = ok ? 1u : 0u;
                if (!ok) (void)ptx_atomic_add64(A.arena_next, 0ull - (unsigned long long)want); /* hand it back: a smaller request of another log may still fit */
                if (ok) {
                    const uint32_t x = 2u - ext_left;
                    H->ext_cap[x] = want;
                    H->ext_lo[x] = (uint32_t)(A.arena_base + at);
                    H->ext_hi[x] = (uint32_t)((A.arena_base + at) >> 32);
                }
            }
            PTX_SYNC_T();
            if (PTX_U32(H->ext_ok)) {
                room += want;
                ext_left -= 1u;
            } else {
                ext_left = 0u; /* the arena is exhausted */
            }
            PTX_SYNC_T();
        }
    }
    PTX_FOR(i, chunk_n) {
        const uint32_t tt = t0 + i, a_ = action[tt];
        uint32_t kind = PTX_RK_SKIP, va = SLOT_NONE, vb = SLOT_NONE;
        if (a_ == PTX_ACT_MAKELIST) {
            kind = PTX_RK_MAKELIST;
        } else if (a_ == PTX_ACT_INSERT) {
            kind = PTX_RK_INSERT;
            va = erank[tt] & PTX_RANK_MASK; /* final rank of the element */
        } else if (a_ == PTX_ACT_DELETE) {
            const uint32_t r = refs[tt]; /* the row that inserted the target (always one, in a log the merge accepted) */
            if (r < N) {
                kind = PTX_RK_DELETE;
                va = erank[r] & PTX_RANK_MASK;
            }
        } else if ((a_ == PTX_ACT_ADDMARK || a_ == PTX_ACT_REMOVEMARK) && mark_type[tt] < 4u) {
            const uint32_t v = refs[tt];
            va = v & 0xFFFFu;
            vb = v >> 16;
            if (n > 32766u) { /* the high halves beside (none: all ones in both) */
                const uint32_t vh = A.refs_hi[base + tt];
                va |= vh << 16;
                vb |= vh & 0xFFFF0000u;
            } else {
                va = va == 0xFFFFu ? SLOT_NONE : va;
                vb = vb == 0xFFFFu ? SLOT_NONE : vb;
            }
            kind = PTX_RK_MARK | ((uint32_t)mark_type[tt] << 4) | (a_ == PTX_ACT_ADDMARK ? 64u : 0u);
        }
        /* (ranks and slots index the slice: one beyond the header's element count — a header that understates it — skips the row instead of writing outside) */
        if ((kind == PTX_RK_INSERT || kind == PTX_RK_DELETE) && va >= n) kind = PTX_RK_SKIP;
        if ((kind & 15u) == PTX_RK_MARK && ((va != SLOT_NONE && va > 2u * n + 1u) || (vb != SLOT_NONE && vb > 2u * n + 1u))) kind = PTX_RK_SKIP;
        c_kind[i] = (uint8_t)kind;
        PtxChunkRow cr;
        cr.id = op_id[tt];
        cr.pay = payload[tt];
        cr.a = va;
        cr.b = vb;
        c_row[i] = cr;
    }
    PTX_SYNC_T();
#pragma nounroll
    for (uint32_t ci = 0; ci < chunk_n; ++ci) {
        const uint32_t t = t0 + ci;
        const bool open = t >= first;  /* the rows before `first` count records (npatch) but write none ... */
        if (t == first) npatch = 0u;   /* ... and the count starts again at the first row asked for */
        const uint32_t kindb = PTX_U32(c_kind[ci]);
        const uint32_t kind = kindb & 15u;
        if (kind == PTX_RK_MAKELIST) {
            PTX_LEADER { ptx_patch_put(dst, open, npatch, t, PTX_PATCH_MAKELIST, 0u, 0u); }
            npatch += 1u;
            continue;
        }
        if (kind == PTX_RK_SKIP) continue;
        PTX_H_FENCE(); /* the state stores of the ops before have landed */
        if (kind == PTX_RK_INSERT) {
            const uint32_t r = PTX_U32(c_row[ci].a);
            const uint32_t l1 = ndef ? PTX_U32(ptx_hbm_last_below(S, 2u * r)) : 0u; /* slot + 1 */
            const uint32_t p0 = npatch;
            uint32_t attr = 0;
            bool coms = false;
            if (l1) { /* the marks of the closest defined slot to the left */
                const uint32_t l = l1 - 1u;
                const uint32_t lw = l >> 5, lb = l & 31u;
                const uint32_t sac = ptx_coherent_load32(&S.mb[lw].ac), s0 = ptx_coherent_load32(&S.mb[lw].on[0]);
                const uint32_t s1 = ptx_coherent_load32(&S.mb[lw].on[1]), s2 = ptx_coherent_load32(&S.mb[lw].on[2]);
                if ((PTX_U32(s0) >> lb) & 1u) attr |= PTX_ATTR_STRONG;
                if ((PTX_U32(s1) >> lb) & 1u) attr |= PTX_ATTR_EM;
                if ((PTX_U32(s2) >> lb) & 1u) attr |= PTX_ATTR_LINK | (PTX_U32(ptx_coherent_load32(&S.lurl[l])) & PTX_ATTR_ID_MASK);
                coms = (PTX_U32(sac) >> lb) & 1u;
                if (coms) attr |= PTX_ATTR_COMMENT;
            }
            const uint32_t vis = PTX_U32(ptx_hbm_rank(S, r));
            PTX_LEADER { ptx_patch_put(dst, open, p0, t, PTX_PATCH_INSERT, vis, attr); }
            uint32_t extra = 0;
            if (coms) {
                const uint32_t l = l1 - 1u;
                PTX_FOR(kc, ncom) {
                    if (PTX_H_BIT(cadd, kc) && ptx_coherent_load32(&ca[kc]) <= l && l < ptx_coherent_load32(&cb[kc])) {
                        bool last = true; /* no later-applied covering op of the same id: the chain of the id, latest first, down to this op */
                        const uint32_t id = ptx_coherent_load16(&ccid[kc]);
                        for (uint32_t y = ptx_coherent_load16(&ctail[id]); y != kc && y != PTX_CHAIN_NONE; y = ptx_coherent_load16(&cprev[y]))
                            if (ptx_coherent_load32(&ca[y]) <= l && l < ptx_coherent_load32(&cb[y])) {
                                last = false;
                                break;
                            }
                        if (last) ptx_patch_put(dst, open, p0 + 1u + ptx_atomic_add(&H->tmp, 1u), t, PTX_PATCH_INSERT_COMMENT, id, 0u);
                    }
                }
                PTX_SYNC_T();
                extra = PTX_U32(H->tmp);
                PTX_SYNC_T();
                PTX_LEADER { H->tmp = 0; }
            }
            ptx_hbm_present_flip<kThreads>(S, r, 1u); /* the element is visible from now on */
            npatch = p0 + 1u + extra;
            PTX_SYNC_T();
        } else if (kind == PTX_RK_DELETE) {
            const uint32_t r = PTX_U32(c_row[ci].a);
            if ((PTX_U32(ptx_coherent_load32(&S.present[r >> 5].bits)) >> (r & 31u)) & 1u) {
                const uint32_t vis = PTX_U32(ptx_hbm_rank(S, r));
                PTX_LEADER { ptx_patch_put(dst, open, npatch, t, PTX_PATCH_DELETE, vis, 1u); }
                npatch += 1u;
                ptx_hbm_present_flip<kThreads>(S, r, 0xFFFFFFFFu);
                PTX_SYNC_T();
            }
        } else if (kind == PTX_RK_MARK) {
            const uint32_t ty = (kindb >> 4) & 3u;
            const bool add = (kindb & 64u) != 0u;
            const PtxChunkRow cr = c_row[ci];
            uint32_t slot_a = PTX_U32(cr.a), slot_b = PTX_U32(cr.b);
            if (slot_a != SLOT_NONE && slot_b == slot_a) slot_b = SLOT_NONE; /* the start test fires first (A.6-3) */
            if (slot_a == SLOT_NONE || slot_b < slot_a) {
                /* the end is met while the op has not started: its slot becomes a defined one, the op covers nothing and the walk stops (peritext.ts:240-243) */
                if (slot_b != SLOT_NONE) PTX_DEFINE_SLOT(slot_b);
                continue;
            }
            PTX_DEFINE_SLOT(slot_a);
            if (slot_b != SLOT_NONE) PTX_DEFINE_SLOT(slot_b); /* inherits the state BEFORE this op from inside the range */
            const uint32_t lim = slot_b != SLOT_NONE ? slot_b : 2u * n;
            const uint32_t wlo = slot_a >> 5, whi = (lim + 31u) >> 5, nw_all = whi > wlo && lim > slot_a ? whi - wlo : 0u;
            const uint32_t my_id = PTX_U32(cr.pay);
            const uint64_t my_op = ((uint64_t)PTX_U32((uint32_t)(cr.id >> 32)) << 32) | PTX_U32((uint32_t)cr.id);
#define PTX_RANGE_MASK(w_) (ptx_span_mask_in(slot_a, lim, (w_))) /* wlo <= w_ < whi */
            /* first defined slot of the range in the words after w_, else the end of the range */
#define PTX_NEXT_AFTER_WORD(w_, out_)                                      \
    uint32_t out_ = ptx_hbm_first_from(S, ((w_) + 1u) << 5);               \
    out_ = out_ < lim ? out_ : lim;
            /* replay_core.h's PTX_FINISH_WORD: of the changed slots ch_ keep those whose patch holds a visible char */
#define PTX_FINISH_WORD(wi_, w_, m_, ch_)                                                                               \
    do {                                                                                                                \
        uint32_t R_ = 0;                                                                                                \
        if (ch_) {                                                                                                      \
            const uint32_t pw_ = ptx_coherent_load32(&S.present[(w_) >> 1].bits);                                       \
            const uint32_t P2_ = ptx_spread16(((w_)&1u) ? pw_ >> 16 : pw_) & PTX_RANGE_MASK(w_);                        \
            uint32_t G_ = P2_ & (m_);                                                                                   \
            const uint32_t Q_ = P2_ & ~(m_);                                                                            \
            if (Q_) {                                                                                                   \
                const uint32_t Dr_ = ptx_brev(m_);                                                                      \
                G_ |= ptx_brev((~Dr_ + ptx_brev(Q_)) & Dr_);                                                            \
            }                                                                                                           \
            const uint32_t top_ = 31u - (uint32_t)__builtin_clz(m_);                                                    \
            if ((((ch_) & ~G_) >> top_) & 1u) {                                                                         \
                PTX_NEXT_AFTER_WORD(w_, nx_)                                                                            \
                if (nx_ > (((w_) + 1u) << 5) && PTX_VIS_AT(nx_) > ptx_hbm_rank(S, ((w_) + 1u) << 4)) G_ |= 1u << top_;  \
            }                                                                                                           \
            R_ = (ch_) & G_;                                                                                            \
        }                                                                                                               \
        cw[wi_] = R_;                                                                                                   \
        cnt[wi_] = ptx_popc(R_);                                                                                        \
    } while (0)
            const uint32_t li = ty == PTX_MARK_STRONG ? 0u : ty == PTX_MARK_EM ? 1u : 2u; /* (LWW types) */
            const bool lww = ty != PTX_MARK_COMMENT;
            const bool fast = lww && my_op > maxop[li]; /* compareOpIds: this op loses at the slots an applied op of its type with a larger id covers */
            const bool per_slot = lww && li == 2u && add; /* the url of every slot the op wins is stored; where the link was on, it decides "changed" */
            uint32_t y0 = PTX_CHAIN_NONE; /* (comments) the last registered op of this op's id */
            if (!lww) y0 = my_id < Kid ? PTX_U32(ptx_coherent_load16(&ctail[my_id])) : (uint32_t)PTX_CHAIN_NONE;
            uint32_t prun = npatch;
            /* the range, PTX_HBM_TILE words at a time: every pass of replay_core.h over one tile, its records behind those of the tiles before */
#pragma nounroll
            for (uint32_t tw = 0; tw < nw_all; tw += PTX_HBM_TILE) {
                const uint32_t w0 = wlo + tw, nw = nw_all - tw < PTX_HBM_TILE ? nw_all - tw : PTX_HBM_TILE;
                if (lww) {
                    if (!fast) {
                        PTX_FOR(wi, nw) cw[wi] = 0u;
                        PTX_SYNC_T();
                        PTX_FOR(e, ntab[li]) {
                            const uint64_t ent = ptx_coherent_load64(&tab[2u * (toff[li] + e)]);
                            if (op_id[(uint32_t)ent] > my_op) {
                                const uint32_t ya = (uint32_t)(ent >> 32), yl = (uint32_t)ptx_coherent_load64(&tab[2u * (toff[li] + e) + 1u]);
                                const uint32_t v0 = (ya >> 5) > w0 ? ya >> 5 : w0, v1 = ((yl + 31u) >> 5) < w0 + nw ? (yl + 31u) >> 5 : w0 + nw;
                                for (uint32_t v = v0; v < v1; ++v) ptx_atomic_or(&cw[v - w0], ptx_span_mask(ya, yl, v));
                            }
                        }
                        PTX_SYNC_T();
                    }
                    PTX_FOR(wi, nw) {
                        const uint32_t w = w0 + wi;
                        const uint32_t m = ptx_coherent_load32(&S.d0[w]) & PTX_RANGE_MASK(w);
                        const uint32_t upd = fast ? m : m & ~cw[wi];
                        uint32_t old = 0;
                        if (m) old = ptx_coherent_load32(&S.mb[w].on[li]);
                        if (upd) ptx_coherent_store32(&S.mb[w].on[li], add ? old | upd : old & ~upd);
                        if (per_slot) {
                            cw[wi] = upd & ~old; /* (the two together: the slots the op wins) */
                            cnt[wi] = upd & old;
                        } else {
                            const uint32_t ch = upd & (add ? ~old : old);
                            PTX_FINISH_WORD(wi, w, m, ch);
                        }
                    }
                    if (per_slot) {
                        PTX_SYNC_T();
                        const uint32_t my_url = my_id & PTX_ATTR_ID_MASK;
                        PTX_FOR(j, nw << 5) {
                            const uint32_t wi = j >> 5, bit = j & 31u;
                            const bool both = (cnt[wi] >> bit) & 1u; /* the link was on: changed iff the urls differ */
                            if (both || ((cw[wi] >> bit) & 1u)) {
                                const uint32_t s = ((w0 + wi) << 5) + bit;
                                if (both && (ptx_coherent_load32(&S.lurl[s]) & PTX_ATTR_ID_MASK) != my_url) ptx_atomic_or(&cw[wi], 1u << bit);
                                ptx_coherent_store32(&S.lurl[s], my_id);
                            }
                        }
                        PTX_SYNC_T();
                        PTX_FOR(wi, nw) {
                            const uint32_t w = w0 + wi;
                            const uint32_t m = ptx_coherent_load32(&S.d0[w]) & PTX_RANGE_MASK(w);
                            const uint32_t ch = cw[wi];
                            PTX_FINISH_WORD(wi, w, m, ch);
                        }
                    }
                } else {
                    /* comments: the last-applied covering op with this id decides (this op is not registered yet): per word, the id's chain latest first */
                    PTX_FOR(wi, nw) {
                        const uint32_t w = w0 + wi;
                        const uint32_t m = ptx_coherent_load32(&S.d0[w]) & PTX_RANGE_MASK(w);
                        uint32_t und = m, onm = 0;
                        for (uint32_t y = y0; y != PTX_CHAIN_NONE && und; y = ptx_coherent_load16(&cprev[y])) {
                            const uint32_t c = ptx_span_mask(ptx_coherent_load32(&ca[y]), ptx_coherent_load32(&cb[y]), w) & und;
                            if (PTX_H_BIT(cadd, y)) onm |= c;
                            und &= ~c;
                        }
                        uint32_t any = 0;
                        if (m) {
                            any = ptx_coherent_load32(&S.mb[w].ac);
                            ptx_coherent_store32(&S.mb[w].ac, any | m);
                        }
                        const uint32_t ch = add ? m & ~onm : m & (onm | ~any); /* remove on no comment key: undefined -> [] */
                        PTX_FINISH_WORD(wi, w, m, ch);
                    }
                }
                PTX_SYNC_T();
                const uint32_t P = ptx_scan_excl<uint32_t, 1, kThreads>(cnt, nw, H->scan_tmp);
                if (P) {
                    PTX_FOR(wi, nw) {
                        uint32_t R = cw[wi];
                        if (R) {
                            const uint32_t w = w0 + wi;
                            const uint32_t m = ptx_coherent_load32(&S.d0[w]) & PTX_RANGE_MASK(w);
                            uint32_t o = prun + cnt[wi];
                            while (R) {
                                const uint32_t b = (uint32_t)__builtin_ctz(R);
                                R &= R - 1u;
                                const uint32_t above = m & ptx_bits_from(b + 1u);
                                uint32_t nxt;
                                if (above) {
                                    nxt = (w << 5) + (uint32_t)__builtin_ctz(above);
                                } else {
                                    PTX_NEXT_AFTER_WORD(w, nx)
                                    nxt = nx;
                                }
                                ptx_patch_put(dst, open, o++, t, add ? PTX_PATCH_ADDMARK : PTX_PATCH_REMOVEMARK, PTX_VIS_AT((w << 5) + b), PTX_VIS_AT(nxt));
                            }
                        }
                    }
                }
                prun += P;
                PTX_SYNC_T(); /* the tile buffers are rewritten next */
            }
            npatch = prun;
            if (lww) { /* the op joins the table of its type */
                if (toff[li] + ntab[li] <= Kl) { /* (always, with the census' header: the table has Kl + 1 entries) */
                    PTX_LEADER {
                        ptx_coherent_store64(&tab[2u * (toff[li] + ntab[li])], (uint64_t)t | ((uint64_t)slot_a << 32));
                        ptx_coherent_store64(&tab[2u * (toff[li] + ntab[li]) + 1u], (uint64_t)lim);
                    }
                    ntab[li] += 1u;
                }
                if (fast) maxop[li] = my_op;
            } else if (my_id < Kid && ncom < Kc) {
                PTX_LEADER {
                    ptx_coherent_store32(&ca[ncom], slot_a);
                    ptx_coherent_store32(&cb[ncom], slot_b);
                    ptx_coherent_store16(&ccid[ncom], (uint16_t)my_id);
                    if (add) ptx_coherent_store32(&cadd[ncom >> 5], ptx_coherent_load32(&cadd[ncom >> 5]) | (1u << (ncom & 31u)));
                    ptx_coherent_store16(&cprev[ncom], (uint16_t)y0);
                    ptx_coherent_store16(&ctail[my_id], (uint16_t)ncom);
                }
                ncom += 1u;
            }
            PTX_SYNC_T();
#undef PTX_FINISH_WORD
#undef PTX_NEXT_AFTER_WORD
#undef PTX_RANGE_MASK
        }
    }
    PTX_SYNC_T(); /* the chunk buffers are rewritten next */
    }
#undef PTX_DEFINE_SLOT
#undef PTX_VIS_AT
#undef PTX_H_BIT
#undef PTX_H_FENCE
    PTX_LEADER {
        ptx_patch_log pl;
        const uint32_t produced = first < N ? npatch : 0u; /* (first >= N: nothing was asked for) */
        pl.status = produced > room ? (uint32_t)PTX_ERR_CAPACITY : (uint32_t)PTX_OK;
        pl.n_patches = produced;
        A.plogs[log] = pl;
        if (A.ext_off) {
            A.ext_off[3 * (uint64_t)log] = H->ext_cap[0] ? ((uint64_t)H->ext_hi[0] << 32) | H->ext_lo[0] : ~0ull;
            A.ext_off[3 * (uint64_t)log + 1] = H->ext_cap[1] ? ((uint64_t)H->ext_hi[1] << 32) | H->ext_lo[1] : ~0ull;
            A.ext_off[3 * (uint64_t)log + 2] = H->ext_cap[0];
        }
    }
}
