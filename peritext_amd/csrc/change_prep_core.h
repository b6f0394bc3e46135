/*
 * change_prep_core.h — what ptx_change does on the host BEFORE its kernel, for InputOperations that are resident (ptx_change_device): the rows every log will
 * make, the check of the inserts against `values`, the check of the two offset arrays, and the size of the launch's LDS.
 *
 * ptx_change walks every InputOperation on the host (rows per log, `payload + count <= n_values`, at most PTX_CHANGE_ROWS_MAX rows), walks chg_off and op_off
 * (start at 0, never decrease) and downloads every ptx_log_hdr and log_off of the base batch to size the LDS.  Here the same is two passes over what already
 * lies in HBM; the host learns one verdict word, two totals and the maximal LDS need.
 *
 *   ptx_change_offsets_check_one   a lane per entry of chg_off and of op_off: entry 0 must be 0, entry i must not be below entry i - 1, and the last entry must
 *                                  be the size the object was made with (ptx_input_ops_upload reads them from these very entries; ptx_input_ops_wrap_device
 *                                  takes them from its caller, and nothing may be read behind the columns it was given).
 *   ptx_change_prep_log            ONE 64-lane wave per log.  A log that makes no Change writes rows = 0, list words = 0 and leaves.  Otherwise the lanes stride
 *                                  over the log's InputOperations op_off[chg_off[l]] .. op_off[chg_off[l + 1]] (the Changes of a log are contiguous) and sum,
 *                                  in 64 bits, rows (one per inserted value, per deleted element, per mark, per makeList or map row) and grow (the inserted
 *                                  values); an insert is tested with payload + count <= n_values in 64 bits.  The sums are reduced across the wave; the leader
 *                                  reads the log's own ptx_log_hdr and log_off, and writes rows[l] and list_words[l] — ptx_change_list_words where
 *                                  ptx_change_lds_need exceeds the context's LDS or every list is asked into HBM, else 0 — and folds the log's LDS need into one
 *                                  device word (a 64-bit max).  A log whose own offsets are out of order or out of range reads nothing behind them: the offsets
 *                                  pass reports it.
 *
 * Errors go into ONE 64-bit word, a min over (code << 56 | log or entry): the lowest code, and of that the lowest log or entry, whatever the order the waves ran
 * in.  The codes follow the order of ptx_change's own checks.  The word starts as all ones: no error.
 *
 * (the host library scans rows and list_words into out_off and list_off with ptx_find_offsets_kernel; ptx_change_kernel then runs unchanged on them)
 *
 * Plain vector loads and stores and atomics only; written against the platform layer like the other cores: hipcc builds it into the product,
 * tests/emu/emu_change_prep.cc plays it on one host thread.
 */
#pragma once
#include "change_core.h"

enum {
    PTX_CP_CHG_START = 1,   /* chg_off must start at 0 */
    PTX_CP_CHG_ORDER = 2,   /* chg_off decreases              (entry) */
    PTX_CP_OP_START = 3,    /* op_off must start at 0 */
    PTX_CP_OP_ORDER = 4,    /* op_off decreases               (entry) */
    PTX_CP_SIZES = 5,       /* chg_off / op_off do not end at the sizes the object was made with   (0: chg_off, 1: op_off) */
    PTX_CP_VALUES = 6,      /* an insert points outside `values`                                   (log) */
    PTX_CP_ROWS = 7         /* more than PTX_CHANGE_ROWS_MAX rows for one log                      (log) */
};
#define PTX_CP_NO_ERROR 0xFFFFFFFFFFFFFFFFull
#define PTX_CP_AT_MASK 0x00FFFFFFFFFFFFFFull
#define PTX_CP_WORD(code_, at_) (((unsigned long long)(code_) << 56) | ((unsigned long long)(at_) & PTX_CP_AT_MASK))

struct PtxChangePrepArgs {
    /* the InputOperations */
    const uint64_t* chg_off;  /* [n_logs + 1] */
    const uint64_t* op_off;   /* [n_changes + 1] */
    const uint8_t* action;    /* [n_input_ops] */
    const uint32_t* count;
    const uint32_t* payload;
    uint64_t n_changes, n_input_ops, n_values;
    uint32_t has_values;      /* `values` is not NULL */
    uint32_t n_logs;
    /* the base batch */
    const uint64_t* log_off;
    const ptx_log_hdr* log_hdr;
    uint32_t max_actors;
    uint32_t all_in_hbm;      /* PTX_CHANGE_LIST_IN_HBM: the element list of EVERY log that makes a Change goes into global scratch */
    uint64_t max_lds;         /* the context's */
    /* output */
    uint32_t* rows;           /* [n_logs] rows log l will make (0 for a log in error) */
    uint32_t* list_words;     /* [n_logs] words of list scratch of log l (0: the list fits the LDS) */
    unsigned long long* err;  /* one word, PTX_CP_NO_ERROR before the passes */
    unsigned long long* lds_need; /* one word, 0 before the passes: the max of ptx_change_lds_need over the logs that make a Change */
};

struct PtxChangePrepHdr {
    unsigned long long rows, grow;
    uint32_t bad, pad[3];
};
#define PTX_CHANGE_PREP_LDS_BYTES 32u
static_assert(sizeof(PtxChangePrepHdr) == PTX_CHANGE_PREP_LDS_BYTES, "the header is the wave's whole LDS");

#if defined(PTX_EMU)
PTX_DEV void ptx_cp_atomic_min64(unsigned long long* p, unsigned long long v) {
    if (v < *p) *p = v;
}
#else
PTX_DEV void ptx_cp_atomic_min64(unsigned long long* p, unsigned long long v) { (void)atomicMin(p, v); }
#endif

/* entry i of the two offset arrays laid end to end: chg_off[0 .. n_logs], then op_off[0 .. n_changes] (none when there is no Change: ptx_change reads none) */
PTX_HD uint64_t ptx_change_offsets_entries(const PtxChangePrepArgs& A) { return A.n_logs ? (uint64_t)A.n_logs + 1u + (A.n_changes ? A.n_changes + 1u : 0u) : 0u; }
PTX_DEV void ptx_change_offsets_check_one(const PtxChangePrepArgs& A, uint64_t i) {
    const uint64_t nl = (uint64_t)A.n_logs + 1u;
    const bool chg = i < nl;
    const uint64_t* off = chg ? A.chg_off : A.op_off;
    const uint64_t k = chg ? i : i - nl, last = chg ? (uint64_t)A.n_logs : A.n_changes;
    const uint64_t v = off[k];
    if (k == 0u) {
        if (v != 0u) ptx_cp_atomic_min64(A.err, PTX_CP_WORD(chg ? PTX_CP_CHG_START : PTX_CP_OP_START, 0u));
    } else if (v < off[k - 1u]) {
        ptx_cp_atomic_min64(A.err, PTX_CP_WORD(chg ? PTX_CP_CHG_ORDER : PTX_CP_OP_ORDER, k));
    }
    if (k == last && v != (chg ? A.n_changes : A.n_input_ops)) ptx_cp_atomic_min64(A.err, PTX_CP_WORD(PTX_CP_SIZES, chg ? 0u : 1u));
}

template <uint32_t kThreads>
PTX_DEV void ptx_change_prep_log(const PtxChangePrepArgs& A, uint32_t l, uint8_t* lds) {
    PtxChangePrepHdr* H = (PtxChangePrepHdr*)lds;
    const uint64_t c0 = A.chg_off[l], c1 = A.chg_off[l + 1u];
    uint64_t q0 = 0, q1 = 0;
    bool sane = c0 <= c1 && c1 <= A.n_changes; /* (else the offsets pass reports it: nothing is read behind op_off) */
    if (sane && c1 > c0) {
        q0 = A.op_off[c0];
        q1 = A.op_off[c1];
        sane = q0 <= q1 && q1 <= A.n_input_ops; /* (the same: nothing is read behind the op columns) */
    }
    if (!sane || c1 == c0) { /* nothing to do for this replica */
        PTX_LEADER {
            A.rows[l] = 0;
            A.list_words[l] = 0;
        }
        return;
    }
    PTX_LEADER {
        H->rows = 0;
        H->grow = 0;
        H->bad = 0;
    }
    PTX_SYNC_T();
    unsigned long long rows = 0, grow = 0;
    uint32_t bad = 0;
    for (uint64_t s0 = q0; s0 < q1; s0 += 0x40000000ull) { /* (a loop of the platform layer counts in 32 bits) */
        const uint32_t ns = (uint32_t)(q1 - s0 < 0x40000000ull ? q1 - s0 : 0x40000000ull);
        PTX_FOR(i, ns) {
            const uint64_t q = s0 + i;
            const uint32_t a = A.action[q];
            if (a == PTX_IN_INSERT) {
                const uint32_t cnt = A.count[q];
                if ((uint64_t)A.payload[q] + cnt > A.n_values || (cnt && !A.has_values)) bad = 1u;
                rows += cnt;
                grow += cnt;
            } else if (a == PTX_IN_DELETE) {
                rows += A.count[q];
            } else {
                rows += 1u;
            }
        }
    }
    ptx_reduce_add64(&H->rows, rows);
    ptx_reduce_add64(&H->grow, grow);
    ptx_reduce_max32(&H->bad, bad);
    PTX_SYNC_T();
    PTX_LEADER {
        const unsigned long long R = H->rows, G = H->grow;
        if (H->bad) ptx_cp_atomic_min64(A.err, PTX_CP_WORD(PTX_CP_VALUES, l));
        if (R > PTX_CHANGE_ROWS_MAX) ptx_cp_atomic_min64(A.err, PTX_CP_WORD(PTX_CP_ROWS, l));
        if (H->bad || R > PTX_CHANGE_ROWS_MAX) {
            A.rows[l] = 0;
            A.list_words[l] = 0;
        } else {
            /* the launch shape: the LDS of the largest working set among the logs that make a Change, as ptx_change sizes it */
            const bool has_rows = A.log_off[l + 1u] > A.log_off[l];
            const ptx_log_hdr hd = A.log_hdr[l];
            const uint64_t ks = has_rows ? ((uint64_t)hd.max_counter + 1u) * ((uint64_t)(hd.max_actor < 4095u ? hd.max_actor : 4095u) + 1u) : 1u;
            const uint64_t n_l = has_rows ? hd.n_ins : 0u;
            const bool in_hbm = A.all_in_hbm || ptx_change_lds_need(n_l, G, ks, A.max_actors) > A.max_lds;
            /* (ptx_change_kernel refuses a log of more than 0x03FFFFFF elements whatever its list lies in: no scratch for it, and the word count fits 32 bits) */
            A.rows[l] = (uint32_t)R;
            A.list_words[l] = in_hbm && n_l + G <= 0x03FFFFFFull ? (uint32_t)ptx_change_list_words(n_l, G) : 0u;
            ptx_atomic_max64(A.lds_need, ptx_change_lds_need(n_l, G, ks, A.max_actors, in_hbm));
        }
    }
}
