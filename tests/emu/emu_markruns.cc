/*
 * Host emulation of the queries by format on a resident text view (peritext_amd/csrc/markrun_core.h) — TEST TOOLING ONLY, like emu_view.cc, which it includes for
 * the view itself, the view's hit passes and the slice passes; it plays markrun_core.h's passes the way the host library's ptx_view_mark_runs,
 * ptx_view_mark_snippets and ptx_view_find_in_marks launch them.
 *
 * Built into tests/emu/libperitext_emu_markruns.so by __graft_entry__.build() and loaded only by tests/test_emu_markruns.py; tests/emu/emu_markruns_main.cc
 * includes this file into a stand-alone sanitizer program.  One host thread plays every wave and every lane, in the order `reverse` selects.  The kernels use no
 * LDS.  The comment intervals and the per-log rows are the RESULT's (capacity layout: a log's rows at the log's own row offset), handed in per call as the library
 * reads them through the view's `r`.
 */
#include "emu_view.cc"

#include "../../peritext_amd/csrc/markrun_core.h"

extern "C" uint32_t ptx_emu_markrun_step(void) { return 64u; }

static int emu_markrun_check(uint32_t mark_type, uint32_t id, int find) { /* the host library's view_mark_check */
    if (mark_type != PTX_MARK_STRONG && mark_type != PTX_MARK_EM && mark_type != PTX_MARK_COMMENT && mark_type != PTX_MARK_LINK) return PTX_ERR_INVALID_ARG;
    if ((mark_type == PTX_MARK_STRONG || mark_type == PTX_MARK_EM) && id != PTX_MARK_ANY_ID) return PTX_ERR_INVALID_ARG;
    if (mark_type == PTX_MARK_LINK && id != PTX_MARK_ANY_ID && id > PTX_ATTR_ID_MASK) return PTX_ERR_INVALID_ARG;
    if (find && mark_type == PTX_MARK_COMMENT && id == PTX_MARK_ANY_ID) return PTX_ERR_INVALID_ARG;
    return 0;
}

static void emu_markrun_args(const EmuView* v, const ptx_cinterval* cints, const ptx_log_result* logs, uint32_t mark_type, uint32_t id, uint32_t cap, PtxMarkRunArgs& A) {
    memset(&A, 0, sizeof(A));
    A.log_off = v->log_off;
    A.spans = v->spans;
    A.cints = cints;
    A.logs = logs;
    A.status = v->status;
    A.span_off = v->off + ((size_t)v->n_logs + 1);
    A.pre_off = v->pre_off;
    A.pre = v->pre;
    A.first_log = v->first_log;
    A.n_logs = v->n_logs;
    A.mark_type = mark_type;
    A.id = id;
    A.cap = cap;
}

/* the count pass and the scan: n_runs [n_logs], run_off [n_logs + 1].  Returns 0, PTX_ERR_INVALID_ARG as the library would, or -1. */
extern "C" int ptx_emu_markrun_count(const EmuView* v, const ptx_cinterval* cints, const ptx_log_result* logs, uint32_t mark_type, uint32_t id, uint32_t cap, int find, int reverse,
                                     uint32_t* n_runs, uint64_t* run_off) {
    if (!v) return PTX_ERR_INVALID_ARG;
    const int bad = emu_markrun_check(mark_type, id, find);
    if (bad) return bad;
    run_off[0] = 0;
    if (v->n_logs == 0) return 0;
    const size_t no = (size_t)v->n_logs + 1;
    uint64_t* two = (uint64_t*)emu_view_block(2 * no * 8); /* the scan kernel's two rows */
    if (!two) return -1;
    PtxMarkRunArgs A;
    emu_markrun_args(v, cints, logs, mark_type, id, cap, A);
    A.n_runs = n_runs;
    A.run_off = two;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < v->n_logs; ++i) ptx_markrun_count_log<0>(A, ptx_emu_ix(i, v->n_logs));
    emu_view_scan2(two, v->n_logs);
    memcpy(run_off, two, no * 8);
    free(two);
    return 0;
}

/* emit and — with run_unit — finish, with win_start the windows as well: every array [run_off[n_logs]], the caller's */
extern "C" int ptx_emu_markrun_emit(const EmuView* v, const ptx_cinterval* cints, const ptx_log_result* logs, uint32_t mark_type, uint32_t id, uint32_t cap, int reverse,
                                    const uint64_t* run_off, uint32_t* run_start, uint32_t* run_end, uint32_t* run_id, uint32_t* run_unit, uint32_t* run_len, uint32_t before,
                                    uint32_t after, uint32_t* win_start, uint32_t* win_end, uint32_t* match_unit) {
    const uint64_t nr = v->n_logs ? run_off[v->n_logs] : 0;
    if (nr == 0) return 0;
    if (nr > 0xFFFFFFFFull) return PTX_ERR_CAPACITY;
    const size_t no = (size_t)v->n_logs + 1;
    uint64_t* two = (uint64_t*)emu_view_block(2 * no * 8);
    if (!two) return -1;
    memcpy(two, run_off, no * 8);
    PtxMarkRunArgs A;
    emu_markrun_args(v, cints, logs, mark_type, id, cap, A);
    A.run_off = two;
    A.n_listed = (uint32_t)nr;
    A.run_start = run_start;
    A.run_end = run_end;
    A.run_id = run_id;
    A.run_unit = run_unit;
    A.run_len = run_len;
    A.before = before;
    A.after = after;
    A.win_start = win_start;
    A.win_end = win_end;
    A.match_unit = match_unit;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < v->n_logs; ++i) ptx_markrun_emit_log<0>(A, ptx_emu_ix(i, v->n_logs));
    if (run_unit)
        for (uint32_t i = 0; i < A.n_listed; ++i) ptx_markrun_finish_one(A, ptx_emu_ix(i, A.n_listed));
    free(two);
    return 0;
}

static void emu_markrun_filter_args(uint32_t n_logs, uint32_t cap, const uint64_t* hit_off, const uint32_t* hit_unit, const uint32_t* hit_start, const uint32_t* hit_end,
                                    const uint64_t* run_off, const uint32_t* run_start, const uint32_t* run_end, PtxMarkFilterArgs& F) {
    memset(&F, 0, sizeof(F));
    F.n_logs = n_logs;
    F.cap = cap;
    F.hit_off = hit_off;
    F.hit_unit = hit_unit;
    F.hit_start = hit_start;
    F.hit_end = hit_end;
    F.run_off = run_off;
    F.run_start = run_start;
    F.run_end = run_end;
}

/* the filter's count pass over the uncapped hits and runs, and ptx_find_offsets_kernel under the cap: n_kept [n_logs], out_off [n_logs + 1] */
extern "C" int ptx_emu_markrun_filter_count(uint32_t n_logs, uint32_t cap, const uint64_t* hit_off, const uint32_t* hit_start, const uint32_t* hit_end, const uint64_t* run_off,
                                            const uint32_t* run_start, const uint32_t* run_end, int reverse, uint32_t* n_kept, uint64_t* out_off) {
    PtxMarkFilterArgs F;
    emu_markrun_filter_args(n_logs, cap, hit_off, nullptr, hit_start, hit_end, run_off, run_start, run_end, F);
    F.n_kept = n_kept;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < n_logs; ++i) ptx_markrun_filter_log<0, false>(F, ptx_emu_ix(i, n_logs));
    uint64_t run = 0;
    for (uint32_t l = 0; l < n_logs; ++l) {
        out_off[l] = run;
        run += n_kept[l] < cap ? n_kept[l] : cap;
    }
    out_off[n_logs] = run;
    return 0;
}

/* ... and its emit pass: out_unit / out_start / out_end [out_off[n_logs]], the caller's */
extern "C" int ptx_emu_markrun_filter_emit(uint32_t n_logs, uint32_t cap, const uint64_t* hit_off, const uint32_t* hit_unit, const uint32_t* hit_start, const uint32_t* hit_end,
                                           const uint64_t* run_off, const uint32_t* run_start, const uint32_t* run_end, int reverse, const uint64_t* out_off, uint32_t* out_unit,
                                           uint32_t* out_start, uint32_t* out_end) {
    if (n_logs == 0 || out_off[n_logs] == 0) return 0;
    PtxMarkFilterArgs F;
    emu_markrun_filter_args(n_logs, cap, hit_off, hit_unit, hit_start, hit_end, run_off, run_start, run_end, F);
    F.out_off = out_off;
    F.out_unit = out_unit;
    F.out_start = out_start;
    F.out_end = out_end;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < n_logs; ++i) ptx_markrun_filter_log<0, true>(F, ptx_emu_ix(i, n_logs));
    return 0;
}
