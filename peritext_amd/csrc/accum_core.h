/*
 * accum_core.h — the CONSUMER side of the patch API on the device: a Patch[] stream (ptx_patch records, include/peritext_hip.h) turned back into the
 * canonical rows of the document it describes, and their digest.
 *
 * What it replaces: accumulatePatches(allPatches), the third assertion of the reference's fuzzer (reference/test/fuzz.ts:245-278: the stream an editor
 * received rebuilds what getTextWithFormatting computes), restated at id level exactly as tests/helpers.py accumulate_patches does — a comment removeMark
 * removes its own id only and leaves the key present.  Streams of any origin: the replay's own (ptx_check_patches accumulates them where they were written;
 * no record is downloaded) or a peer's (ptx_accumulate_patches).
 *
 * State of a log (C = its insert rows = the most characters a stream of it can insert, Kid = its comment ids):
 *   ser[C]      the visible characters in document order, each named by its SERIAL = its insert ordinal, never reused.  The one array an insert or a delete
 *               shifts: 64 entries at a time through a chunk buffer, from the top chunk down for an insert and from the bottom up for a delete, so that a
 *               chunk is read before it is overwritten
 *   val[C], attr[C]   value id and attr word (PTX_ATTR_* | link url id) by serial: they never move
 *   cbits[Kid][ceil(C / 32)]   comment membership, one bitmap row per id over serials: set / cleared with atomics by the lanes of a mark's range; never moves
 *   brk[C / 32 + 2]   the end phase's span breaks, a bit per visible index
 * A mark record is one pass over [a, b), a lane per character.  The end phase writes the values, walks the visible characters once per comment id (intervals
 * come out sorted by (id, start); a change of membership is a span break), then turns the break bits into span rows with a ballot prefix.
 *
 * One wave per log, as the replay.  ptx_accum_walk is ONE body over two state stores (the pattern of replay_hbm_core.h): PtxAccumLdsStore keeps the state in
 * the log's LDS window, PtxAccumHbmStore in a slice of global scratch (workgroup-scope accessors, a wait for the wave's stores at the head of every record);
 * the bitmap words, which atomics write at the L2, are read back there by the HBM store.  The records, and the payload / action / mark type of their rows, are
 * fetched 64 at a time, a lane each; the walk itself is uniform.
 *
 * Nothing is written outside the log's state and its output rows whatever a record says: every index is checked against the current length (PTX_ERR_INDEX_OOB),
 * every row and id against the log (PTX_ERR_BAD_OP), every output row against the log's row range (PTX_ERR_CAPACITY) BEFORE the record is applied.
 *
 * Compiled two ways like the other kernel sources (hipcc: ptx_accum_kernel / ptx_accum_kernel_hbm; g++ -DPTX_EMU: tests/emu/emu_accum.cc).
 */
#pragma once
#include "merge_core.h"

#define PTX_ACCUM_NONE 0xFFFFFFFFu
#define PTX_ACCUM_KIND_MAX 5u /* PTX_PATCH_INSERT_COMMENT */

struct PtxAccumArgs {
    /* the batch (resident) */
    const uint64_t* log_off;
    const uint32_t* payload;
    const uint8_t* action;
    const uint8_t* mark_type;
    const ptx_log_hdr* log_hdr;
    /* the streams: records of log l at patches[rec_off[l] - rec_base ..), plogs[l].n_patches of them; a log whose plogs[l].status is not PTX_OK has none */
    const ptx_patch* patches;
    const uint64_t* rec_off;
    uint64_t rec_base;
    const ptx_patch_log* plogs;
    /* this launch: workgroup k takes log first_log + k, or log_index[k] when that is set */
    uint32_t first_log, n_launch;
    const uint32_t* log_index;
    /* outputs: the per-log row, and the canonical rows at row offset log_off[l] (all three NULL: counts and digest only) */
    ptx_log_result* res;
    uint32_t* out_values;
    ptx_span* out_spans;
    ptx_cinterval* out_cints;
    /* the comparison of ptx_check_patches (both NULL: none): want[l] = the merge's row of log l */
    const ptx_log_result* want;
    ptx_patch_check_log* check;
    /* HBM store: the state slice of workgroup k is state[state_off[k] .. state_off[k + 1]) (u32 units) */
    uint32_t* state;
    const uint64_t* state_off;
    uint32_t lds_bytes;
};

struct PtxAccumHdr {
    unsigned long long h1, h2; /* the digest */
    uint32_t buf[64];          /* a chunk of `ser` on its way up or down */
    ptx_patch crec[64];        /* 64 records, and of the row of each: */
    uint32_t cpay[64];         /* payload */
    uint32_t cam[64];          /* action | mark_type << 8; PTX_ACCUM_NONE: the row is not of the log */
};

/* where the arrays of a log's state start (u32 units, every array 16-byte aligned) */
struct PtxAccumLayout {
    uint64_t ser, val, attr, brk, cbits, end;
    uint32_t W;
};
PTX_HD uint64_t ptx_accum_a4(uint64_t units) { return (units + 3u) & ~3ull; }
PTX_HD PtxAccumLayout ptx_accum_layout(uint64_t C, uint64_t Kid) {
    PtxAccumLayout L;
    L.W = (uint32_t)((C + 31u) >> 5);
    uint64_t o = 0;
    L.ser = o, o += ptx_accum_a4(C + 1);
    L.val = o, o += ptx_accum_a4(C + 1);
    L.attr = o, o += ptx_accum_a4(C + 1);
    L.brk = o, o += ptx_accum_a4((C >> 5) + 2);
    L.cbits = o, o += ptx_accum_a4(Kid * (uint64_t)L.W);
    L.end = o;
    return L;
}
/* characters a stream of the log can insert: its insert rows */
PTX_HD uint64_t ptx_accum_chars(uint64_t rows, const ptx_log_hdr& h) { return h.n_ins < rows ? h.n_ins : rows; }
/* u32 units of state a log takes (the HBM store's slice) and the LDS window of the LDS store */
PTX_HD uint64_t ptx_accum_units_hdr(uint64_t rows, const ptx_log_hdr& h) { return ptx_accum_layout(ptx_accum_chars(rows, h), h.n_comment_ids).end; }
PTX_HD uint64_t ptx_accum_lds_need_hdr(uint64_t rows, const ptx_log_hdr& h) { return ptx_a16(sizeof(PtxAccumHdr)) + 4 * ptx_accum_units_hdr(rows, h); }
#define PTX_ACCUM_HBM_LDS_BYTES ((uint32_t)((sizeof(PtxAccumHdr) + 15u) & ~15u))

/* ---- the two state stores ---- */
struct PtxAccumState {
    uint32_t *ser, *val, *attr, *brk, *cbits;
    uint32_t W;
    uint64_t units;
    PTX_MEM void point(uint32_t* g, const PtxAccumLayout& Lo) {
        ser = g + Lo.ser, val = g + Lo.val, attr = g + Lo.attr, brk = g + Lo.brk, cbits = g + Lo.cbits;
        W = Lo.W;
        units = Lo.end;
    }
};
/* the state in the log's LDS window behind the header */
struct PtxAccumLdsStore : PtxAccumState {
    PTX_MEM bool place(uint8_t* lds, uint32_t lds_bytes, uint64_t C, uint64_t Kid) {
        const PtxAccumLayout Lo = ptx_accum_layout(C, Kid);
        point((uint32_t*)(lds + ptx_a16(sizeof(PtxAccumHdr))), Lo);
        return ptx_a16(sizeof(PtxAccumHdr)) + 4 * Lo.end <= (uint64_t)lds_bytes;
    }
    PTX_MEM uint32_t ld(const uint32_t* p) const { return *p; }
    PTX_MEM void st(uint32_t* p, uint32_t v) const { *p = v; }
    PTX_MEM void bits_or(uint32_t* p, uint32_t m) const { ptx_atomic_or(p, m); }
    PTX_MEM void bits_clear(uint32_t* p, uint32_t m) const { ptx_atomic_and(p, ~m); }
    PTX_MEM uint32_t bits(uint32_t* p) const { return *p; }
    PTX_MEM void sync() const { PTX_WSYNC(); } /* the wave's LDS accesses before it are ordered before those behind it */
};
/* the state in the log's slice of global scratch */
struct PtxAccumHbmStore : PtxAccumState {
    uint32_t* g;
    uint64_t have;
    PTX_MEM bool place(uint8_t*, uint32_t lds_bytes, uint64_t C, uint64_t Kid) {
        const PtxAccumLayout Lo = ptx_accum_layout(C, Kid);
        point(g, Lo);
        return Lo.end <= have && sizeof(PtxAccumHdr) <= (uint64_t)lds_bytes; /* a slice that is too small (never from this library's host) is refused, not overrun */
    }
    PTX_MEM uint32_t ld(const uint32_t* p) const { return ptx_coherent_load32(p); }
    PTX_MEM void st(uint32_t* p, uint32_t v) const { ptx_coherent_store32(p, v); }
    PTX_MEM void bits_or(uint32_t* p, uint32_t m) const { ptx_atomic_or(p, m); }
    PTX_MEM void bits_clear(uint32_t* p, uint32_t m) const { ptx_atomic_and(p, ~m); }
    PTX_MEM uint32_t bits(uint32_t* p) const { return ptx_l2_load32(p); } /* where the atomics wrote it (behind sync(): they have completed) */
    PTX_MEM void sync() const {
        ptx_global_stores_done();
        PTX_WSYNC();
    }
};

/* L[dst .. dst + (hi - lo)) = L[lo .. hi) for hi - lo <= 64, through the chunk buffer: every entry is read before any is written */
template <uint32_t kThreads, class Store>
PTX_DEV void ptx_accum_move(const Store& S, uint32_t* L, uint32_t lo, uint32_t hi, uint32_t dst, uint32_t* buf) {
    PTX_FOR(l, hi - lo) buf[l] = S.ld(&L[lo + l]);
    PTX_WSYNC();
    PTX_FOR(l, hi - lo) S.st(&L[dst + l], buf[l]);
    PTX_WSYNC();
}
PTX_DEV uint64_t ptx_accum_below(uint32_t l) { return l ? (~0ull >> (64u - l)) : 0ull; } /* the lanes below lane l < 64 */
PTX_DEV uint32_t ptx_accum_popc64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

/* does serial s hold the id whose bitmap row this is */
template <class Store>
PTX_DEV bool ptx_accum_has(const Store& S, uint32_t* row, uint32_t s) { return ((S.bits(&row[s >> 5]) >> (s & 31u)) & 1u) != 0u; }

template <uint32_t kThreads, class Store>
PTX_DEV void ptx_accum_walk(const PtxAccumArgs& A, uint32_t k, uint8_t* lds, uint32_t lds_bytes, Store& S) {
    PtxAccumHdr* H = (PtxAccumHdr*)lds;
    const uint32_t log = A.log_index ? A.log_index[k] : A.first_log + k;
    const uint64_t base = A.log_off[log];
    const uint32_t N = (uint32_t)(A.log_off[log + 1] - base);
    const ptx_log_hdr hd = A.log_hdr[log];
    const uint32_t C = (uint32_t)ptx_accum_chars(N, hd), Kid = hd.n_comment_ids;
    const ptx_patch_log pl = A.plogs[log];
    uint32_t status = pl.status, bad = PTX_ACCUM_NONE;
    const uint32_t P = status == PTX_OK ? pl.n_patches : 0u;
    const ptx_patch* recs = A.patches + (A.rec_off[log] - A.rec_base);
    if (status == PTX_OK && (!S.place(lds, lds_bytes, C, Kid) || (uint64_t)Kid * ((C + 31u) >> 5) > 0xFFFFFFFFull)) status = PTX_ERR_CAPACITY;

    uint32_t len = 0, nser = 0, last = 0;
    bool after_insert = false;
    if (status == PTX_OK) {
        /* nothing is zeroed by the host: the bitmap rows (a new serial's column must read empty), the digest */
        PTX_FOR(i, (uint32_t)((uint64_t)Kid * S.W)) S.st(&S.cbits[i], 0u);
        PTX_LEADER { H->h1 = 0, H->h2 = 0; }
        S.sync();
    }
    for (uint32_t c0 = 0; c0 < P && status == PTX_OK; c0 += 64u) {
        const uint32_t m = P - c0 < 64u ? P - c0 : 64u;
        PTX_FOR(l, m) {
            const ptx_patch r = recs[c0 + l];
            uint32_t pay = 0, am = PTX_ACCUM_NONE;
            if (r.row < N) {
                pay = A.payload[base + r.row];
                am = (uint32_t)A.action[base + r.row] | ((uint32_t)A.mark_type[base + r.row] << 8);
            }
            H->crec[l] = r;
            H->cpay[l] = pay;
            H->cam[l] = am;
        }
        PTX_WSYNC();
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t kind = PTX_U32(H->crec[j].kind), a = PTX_U32(H->crec[j].a), b = PTX_U32(H->crec[j].b), pay = PTX_U32(H->cpay[j]), am = PTX_U32(H->cam[j]);
            const uint32_t act = am & 255u, mt = (am >> 8) & 255u;
            const bool is_mark = kind == PTX_PATCH_ADDMARK || kind == PTX_PATCH_REMOVEMARK;
            /* ---- the record against the log and the document as it stands; nothing has been written for it yet ---- */
            uint32_t err = PTX_OK;
            if (kind > PTX_ACCUM_KIND_MAX || am == PTX_ACCUM_NONE) err = PTX_ERR_BAD_OP;
            else if (kind == PTX_PATCH_INSERT_COMMENT && (!after_insert || a >= Kid)) err = PTX_ERR_BAD_OP;
            else if (is_mark && ((act != PTX_ACT_ADDMARK && act != PTX_ACT_REMOVEMARK) || mt > PTX_MARK_LINK || (mt == PTX_MARK_COMMENT && pay >= Kid))) err = PTX_ERR_BAD_OP;
            else if (kind == PTX_PATCH_INSERT && a > len) err = PTX_ERR_INDEX_OOB;
            else if (kind == PTX_PATCH_DELETE && (uint64_t)a + b > (uint64_t)len) err = PTX_ERR_INDEX_OOB;
            else if (is_mark && (b > len || a > b)) err = PTX_ERR_INDEX_OOB;
            else if (kind == PTX_PATCH_INSERT && nser >= C) err = PTX_ERR_CAPACITY;
            if (err != PTX_OK) {
                status = err;
                bad = c0 + j;
                break;
            }
            S.sync(); /* what the records before wrote */
            if (kind == PTX_PATCH_INSERT) {
                for (uint32_t hi = len; hi > a;) { /* the tail moves up by one, top chunk first */
                    const uint32_t lo = hi - a > 64u ? hi - 64u : a;
                    ptx_accum_move<kThreads>(S, S.ser, lo, hi, lo + 1u, H->buf);
                    hi = lo;
                }
                PTX_LEADER {
                    S.st(&S.ser[a], nser);
                    S.st(&S.val[nser], pay);
                    S.st(&S.attr[nser], b);
                }
                last = nser;
                nser += 1u;
                len += 1u;
            } else if (kind == PTX_PATCH_INSERT_COMMENT) {
                PTX_LEADER { S.bits_or(&S.cbits[(uint64_t)a * S.W + (last >> 5)], 1u << (last & 31u)); }
            } else if (kind == PTX_PATCH_DELETE) {
                for (uint32_t lo = a + b; lo < len && b; lo += 64u) { /* the tail moves down by b, bottom chunk first */
                    const uint32_t hi = len - lo > 64u ? lo + 64u : len;
                    ptx_accum_move<kThreads>(S, S.ser, lo, hi, lo - b, H->buf);
                }
                len -= b;
            } else if (is_mark) {
                const bool add = kind == PTX_PATCH_ADDMARK;
                PTX_FOR(i, b - a) {
                    const uint32_t s = S.ld(&S.ser[a + i]);
                    uint32_t x = S.ld(&S.attr[s]);
                    if (mt == PTX_MARK_COMMENT) {
                        x |= PTX_ATTR_COMMENT; /* a removeMark leaves the key present, possibly [] */
                        uint32_t* wd = &S.cbits[(uint64_t)pay * S.W + (s >> 5)];
                        if (add) S.bits_or(wd, 1u << (s & 31u));
                        else S.bits_clear(wd, 1u << (s & 31u));
                    } else if (mt == PTX_MARK_LINK) {
                        x = add ? ((x & PTX_ATTR_COMMENT) | (x & (PTX_ATTR_STRONG | PTX_ATTR_EM)) | PTX_ATTR_LINK | (pay & PTX_ATTR_ID_MASK)) : (x & ~(PTX_ATTR_LINK | PTX_ATTR_ID_MASK));
                    } else {
                        const uint32_t f = mt == PTX_MARK_STRONG ? PTX_ATTR_STRONG : PTX_ATTR_EM;
                        x = add ? (x | f) : (x & ~f);
                    }
                    S.st(&S.attr[s], x);
                }
            }
            after_insert = kind == PTX_PATCH_INSERT || kind == PTX_PATCH_INSERT_COMMENT;
        }
        PTX_WSYNC(); /* the chunk's records have been read: the next fetch may overwrite them */
    }

    /* ---- the end phase: values, comment intervals (and the breaks they make), spans ---- */
    uint32_t nS = 0, nI = 0;
    const uint32_t n = len;
    if (status == PTX_OK) {
        S.sync();
        uint64_t h1 = 0, h2 = 0;
        PTX_FOR(w, (n >> 5) + 2u) S.st(&S.brk[w], 0u);
        S.sync();
        PTX_FOR(i, n) {
            const uint32_t s = S.ld(&S.ser[i]), v = S.ld(&S.val[s]);
            if (A.out_values) A.out_values[base + i] = v;
            ptx_digest_item(h1, h2, 1u, i, v, 0u);
            if (i == 0u || S.ld(&S.attr[S.ld(&S.ser[i - 1u])]) != S.ld(&S.attr[s])) S.bits_or(&S.brk[i >> 5], 1u << (i & 31u));
        }
        S.sync();
        for (uint32_t c = 0; c < Kid; ++c) {
            uint32_t* row = S.cbits + (uint64_t)c * S.W;
            uint32_t open_start = 0;
            uint64_t carry = 0; /* the character before the chunk holds the id */
            for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
                PTX_BALLOT64(cur, l, i0 + l < n && ptx_accum_has(S, row, S.ld(&S.ser[i0 + l])))
                const uint64_t prev = (cur << 1) | carry, starts = cur & ~prev, ends = ~cur & prev, flips = cur ^ prev;
                if (flips) {
                    PTX_FOR(l, 64u) {
                        /* a change of membership is a span break (a flip at index n, behind the last character, is never read) */
                        if (l < 2u && (uint32_t)(flips >> (32u * l)) != 0u) S.bits_or(&S.brk[(i0 >> 5) + l], (uint32_t)(flips >> (32u * l)));
                        if ((ends >> l) & 1ull) {
                            const uint64_t sb = starts & ptx_accum_below(l);
                            const uint32_t at = nI + ptx_accum_popc64(ends & ptx_accum_below(l)), st = sb ? i0 + 63u - (uint32_t)__builtin_clzll(sb) : open_start;
                            if (at < N && A.out_cints) {
                                ptx_cinterval ci;
                                ci.id = c, ci.start = st, ci.end = i0 + l;
                                A.out_cints[base + at] = ci;
                            }
                            ptx_digest_item(h1, h2, 3u, c, st, i0 + l);
                        }
                    }
                    nI += ptx_accum_popc64(ends);
                    if (starts) open_start = i0 + 63u - (uint32_t)__builtin_clzll(starts);
                }
                carry = cur >> 63;
            }
            if (carry) { /* the id holds to the end of a text of a multiple of 64 characters */
                PTX_LEADER {
                    if (nI < N && A.out_cints) {
                        ptx_cinterval ci;
                        ci.id = c, ci.start = open_start, ci.end = n;
                        A.out_cints[base + nI] = ci;
                    }
                    ptx_digest_item(h1, h2, 3u, c, open_start, n);
                }
                nI += 1u;
            }
        }
        S.sync();
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            PTX_BALLOT64(brks, l, i0 + l < n && ((S.bits(&S.brk[(i0 + l) >> 5]) >> ((i0 + l) & 31u)) & 1u) != 0u)
            if (brks) {
                PTX_FOR(l, 64u) {
                    if ((brks >> l) & 1ull) {
                        const uint32_t at = nS + ptx_accum_popc64(brks & ptx_accum_below(l));
                        ptx_span sp;
                        sp.start = i0 + l;
                        sp.attr = S.ld(&S.attr[S.ld(&S.ser[i0 + l])]);
                        if (at < N && A.out_spans) A.out_spans[base + at] = sp;
                        ptx_digest_item(h1, h2, 2u, at, sp.start, sp.attr);
                    }
                }
                nS += ptx_accum_popc64(brks);
            }
        }
        if (nI > N || nS > N || n > N) status = PTX_ERR_CAPACITY; /* more rows than the log's row range holds */
        PTX_LEADER {
            ptx_digest_item(h1, h2, 4u, 0u, n, nS);
            ptx_digest_item(h1, h2, 4u, 1u, nI, nser);
        }
        if ((h1 | h2) != 0ull) {
            ptx_atomic_add64(&H->h1, (unsigned long long)h1);
            ptx_atomic_add64(&H->h2, (unsigned long long)h2);
        }
        PTX_WSYNC();
    }
    PTX_LEADER {
        const bool ok = status == PTX_OK;
        ptx_log_result R;
        R.status = status;
        R.n_ops = ok ? P : 0u;
        R.n_elems = ok ? nser : 0u;
        R.n_visible = ok ? n : 0u;
        R.n_spans = ok ? nS : 0u;
        R.n_cintervals = ok ? nI : 0u;
        R.reserved[0] = (uint32_t)(4u * S.units);
        R.reserved[1] = bad;
        R.digest[0] = ok ? (uint64_t)H->h1 : 0ull;
        R.digest[1] = ok ? (uint64_t)H->h2 : 0ull;
        if (A.res) A.res[log] = R;
        if (A.check) {
            const ptx_log_result Wt = A.want[log];
            ptx_patch_check_log Ck;
            Ck.status = status;
            Ck.agrees = ok && Wt.status == PTX_OK && Wt.n_elems == R.n_elems && Wt.n_visible == R.n_visible && Wt.n_spans == R.n_spans && Wt.n_cintervals == R.n_cintervals &&
                                Wt.digest[0] == R.digest[0] && Wt.digest[1] == R.digest[1]
                            ? 1u
                            : 0u;
            Ck.n_patches = pl.n_patches;
            Ck.first_bad_record = bad;
            Ck.digest[0] = R.digest[0];
            Ck.digest[1] = R.digest[1];
            A.check[log] = Ck;
        }
    }
}

/* workgroup k of a launch: the state in the LDS window ... */
template <uint32_t kThreads>
PTX_DEV void ptx_accum_log(const PtxAccumArgs& A, uint32_t k, uint8_t* lds) {
    PtxAccumLdsStore S;
    S.units = 0;
    ptx_accum_walk<kThreads>(A, k, lds, A.lds_bytes, S);
}
/* ... or in its slice of global scratch */
template <uint32_t kThreads>
PTX_DEV void ptx_accum_log_hbm(const PtxAccumArgs& A, uint32_t k, uint8_t* lds) {
    PtxAccumHbmStore S;
    S.units = 0;
    S.g = A.state + A.state_off[k];
    S.have = A.state_off[k + 1] - A.state_off[k];
    ptx_accum_walk<kThreads>(A, k, lds, PTX_ACCUM_HBM_LDS_BYTES, S);
}
