/*
 * replay_hbm_core.h — the patch stream of a replica log whose replay state does not fit one CU's LDS (beside replay_core.h as biglog_core.h sits beside
 * merge_core.h).
 *
 * Not a second replay: ptx_replay_log_hbm runs replay_core.h's ptx_replay_walk, the one walk the LDS builds run too, over PtxReplayHbmStore — this file is that
 * store and what it stands on (the slice layout and its sizes, the searches, the kernel's arguments).  The records and their order are those of
 * ptx_replay_log<T, true, true> (32-bit ranks and slots); what changes is where the state lives: every array whose size grows with the document (n, K, Kc, Kid) is
 * in a slice of global scratch sized by ptx_replay_hbm_units_hdr, read and written with the workgroup-scope accessors (ptx_coherent_*), with a wait for the wave's
 * outstanding stores (ptx_global_stores_done) at the head of every op and after a slot has been defined.  The LDS holds what does not grow: the header, the 32-row
 * chunk buffers, ONE TILE of the per-word cw / cnt of a mark op (PTX_HBM_TILE words; the walk works a longer range through tile by tile, the record count carried
 * across), and the top levels of the two summaries below (bounded by n <= 0x03FFFFFF).  One 64-thread workgroup (one wave) per log, as replay_core.h.
 *
 * Three operations of the LDS store walk the whole state per op and would be quadratic in HBM; here they are:
 *   visible index (present[w].pre +- 1 for every word above the rank)
 *       -> THREE levels of prefixes: present[w].pre counts from the start of the word's BLOCK of 64 words, bpre[b] from the start of the block's SUPERBLOCK of
 *          64 blocks (both in HBM), spre[s] from the start of the document (LDS, at most 513 entries).  rank = spre + bpre + pre + popcount of the bits below:
 *          three independent loads, by any lane.  An insert / delete rewrites one word, the at most 63 prefixes behind it in its block (one load and one store
 *          per lane), the at most 63 behind its block in the superblock, and the LDS entries.
 *   closest defined slot to the left (ptx_last_set_below: 64 words per step from the top down)
 *       -> a summary per level, "word i of the level below is non-zero": d1 over defined, d2 over d1 (HBM), d3 over d2 (LDS, at most 129 words).  The search
 *          climbs while the masked word of a level is empty and descends through the highest bit: at most six dependent loads, one when the word that holds
 *          the slot has a defined one below it; none at all while nothing is defined (a counter in a register).
 *   next defined slot of the range (the LDS store's next_defined: word by word upwards)
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
    uint32_t *defined, *d1, *d2, *d3; /* `defined` and its summaries (d0 .. d3 of the layout) */
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
    uint32_t w = (lim - 1u) >> 5, m = ptx_coherent_load32(&S.defined[w]) & ptx_bits_below(((lim - 1u) & 31u) + 1u);
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
    hit = (hit << 5) + ptx_hbm_top_bit(ptx_coherent_load32(&S.defined[hit]));
    return hit + 1u;
}
/* the lowest defined slot at or above `pos`, PTX_HBM_NONE when there is none (any lane) */
PTX_DEV uint32_t ptx_hbm_first_from(const PtxHbmState& S, uint32_t pos) {
    uint32_t w = pos >> 5;
    if (w >= S.nw0) return PTX_HBM_NONE;
    uint32_t m = ptx_coherent_load32(&S.defined[w]) & ptx_bits_from(pos & 31u);
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
    return (hit << 5) + (uint32_t)__builtin_ctz(ptx_coherent_load32(&S.defined[hit]));
}
/* ONE lane: slot s becomes a defined one (the summaries follow where its word was empty) */
PTX_DEV void ptx_hbm_set_defined(const PtxHbmState& S, uint32_t s) {
    uint32_t i = s >> 5;
    uint32_t old = ptx_coherent_load32(&S.defined[i]);
    ptx_coherent_store32(&S.defined[i], old | (1u << (s & 31u)));
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

/* The state in the log's slice of global scratch (32-bit ranks and slots, as the wide LDS build): everything is reached with the workgroup-scope accessors; the
 * wave waits for its own stores at the head of every op and after a slot is defined, nowhere in between.  kTile words of cw / cnt in the LDS. */
struct PtxReplayHbmStore : PtxHbmState {
    static constexpr bool kWide = true;
    static constexpr uint32_t kTile = PTX_HBM_TILE;
    typedef uint32_t slot_t;
    uint32_t* g;     /* the log's slice ... */
    uint64_t units;  /* ... and its size in u32 */
    uint32_t zero_n; /* [g, g + zero_n) must read zero when the replay starts */
    uint32_t ndef;   /* defined slots so far (the same value in every lane): no search while there is none */
    uint64_t* tab;   /* applied LWW mark op: {row | start slot << 32, end of its interval} */
    uint32_t *ca, *cb, *cadd;
    uint16_t *cprev, *ccid, *ctail;

    PTX_MEM bool place(PtxBump& bp, const PtxReplayArgs& A, uint32_t n, uint32_t, uint32_t Kl, uint32_t Kc, uint32_t Kid) {
        const PtxHbmLayout Lo = ptx_replay_hbm_layout(n, (uint64_t)Kl + Kc, Kc, Kid);
        present = (PtxBitWord*)(g + Lo.present);
        bpre = g + Lo.bpre;
        defined = g + Lo.d0;
        d1 = g + Lo.d1;
        d2 = g + Lo.d2;
        nwe = Lo.nwe, nblk = Lo.nblk, nsup = Lo.nsup, nw0 = Lo.nw0, nw1 = Lo.nw1, nw2 = Lo.nw2, nw3 = Lo.nw3;
        mb = (PtxMarkBits*)(g + Lo.mb);
        lurl = g + Lo.lurl;
        cadd = g + Lo.cadd;
        tab = (uint64_t*)(g + Lo.tab);
        ca = g + Lo.ca;
        cb = g + Lo.cb;
        cprev = (uint16_t*)(g + Lo.cprev);
        ccid = (uint16_t*)(g + Lo.ccid);
        ctail = (uint16_t*)(g + Lo.ctail);
        zero_n = (uint32_t)(Lo.zero_end - Lo.present);
        spre = ptx_alloc<uint32_t>(bp, PTX_HBM_SUP_MAX);
        d3 = ptx_alloc<uint32_t>(bp, PTX_HBM_D3_MAX);
        /* a result without the slots' high halves cannot say where the marks of a log of more than 32 766 elements are; a slice that is too small (never from
         * this library's host) is refused, not overrun */
        return !(n > 32766u && !A.refs_hi) && units >= Lo.end && Lo.nsup <= PTX_HBM_SUP_MAX && Lo.nw3 <= PTX_HBM_D3_MAX;
    }
    template <uint32_t kThreads>
    PTX_MEM void reset(uint32_t) { /* the slice is not zeroed by the host */
        PTX_FOR(i, zero_n) ptx_coherent_store32(&g[i], 0u);
        PTX_FOR(i, PTX_HBM_SUP_MAX) spre[i] = 0u;
        PTX_FOR(i, PTX_HBM_D3_MAX) d3[i] = 0u;
        ndef = 0u;
        ptx_global_stores_done();
    }
    template <class T> PTX_MEM T ld(const T* p) const { return ptx_coherent_load(p); }
    template <class T> PTX_MEM void st(T* p, T v) const { ptx_coherent_store(p, v); }
    template <class T> PTX_MEM T ldw(const T* p) const { return ptx_coherent_load(p); }
    template <class T> PTX_MEM void stw(T* p, T v) const { ptx_coherent_store(p, v); }
    PTX_MEM PtxMarkBits load_mb(uint32_t w) const {
        PtxMarkBits v;
        v.ac = ptx_coherent_load32(&mb[w].ac), v.on[0] = ptx_coherent_load32(&mb[w].on[0]);
        v.on[1] = ptx_coherent_load32(&mb[w].on[1]), v.on[2] = ptx_coherent_load32(&mb[w].on[2]);
        return v;
    }
    PTX_MEM void store_mb(uint32_t w, const PtxMarkBits& v) const {
        ptx_coherent_store32(&mb[w].ac, v.ac), ptx_coherent_store32(&mb[w].on[0], v.on[0]);
        ptx_coherent_store32(&mb[w].on[1], v.on[1]), ptx_coherent_store32(&mb[w].on[2], v.on[2]);
    }
    PTX_MEM void op_head() const { ptx_global_stores_done(); } /* the state stores of the ops before have landed */
    PTX_MEM void slot_defined() {
        ndef += 1u;
        ptx_global_stores_done();
    }
    PTX_MEM void before_read() const {}
    PTX_MEM uint32_t rank(uint32_t pos) const { return ptx_hbm_rank(*this, pos); }
    template <uint32_t kThreads>
    PTX_MEM void present_set(uint32_t r, bool on) const { ptx_hbm_present_flip<kThreads>(*this, r, on ? 1u : 0xFFFFFFFFu); }
    PTX_MEM uint32_t last_defined_below(uint32_t lim) const { return ndef ? ptx_hbm_last_below(*this, lim) : 0u; }
    PTX_MEM uint32_t next_defined(uint32_t w, uint32_t, uint32_t lim, uint32_t) const {
        const uint32_t s = ptx_hbm_first_from(*this, (w + 1u) << 5);
        return s < lim ? s : lim;
    }
    PTX_MEM void set_defined(uint32_t s) const { ptx_hbm_set_defined(*this, s); }
};

/* the k-th log of the launch: ptx_replay_walk (replay_core.h) over its slice */
template <uint32_t kThreads>
PTX_DEV void ptx_replay_log_hbm(const PtxReplayHbmArgs& HA, uint32_t k, uint8_t* lds) {
    PtxReplayHbmStore S;
    S.g = HA.state + HA.state_off[k];
    S.units = HA.state_off[k + 1] - HA.state_off[k];
    ptx_replay_walk<kThreads>(HA.R, HA.log_index[k], lds, PTX_REPLAY_HBM_LDS_BYTES, S);
}
