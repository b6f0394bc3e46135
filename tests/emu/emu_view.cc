/*
 * Host emulation of the resident text view (peritext_amd/csrc/view_core.h) — TEST TOOLING ONLY, like emu_find.cc and emu_slice.cc; it includes emu_text.cc for the
 * text passes and plays find_core.h's and slice_core.h's passes itself, over the view's arrays, the way the host library's view queries launch them.
 *
 * Built into tests/emu/libperitext_emu_view.so by __graft_entry__.build() and loaded only by tests/test_emu_view.py; tests/emu/emu_view_main.cc includes this file
 * into a stand-alone sanitizer program.  One host thread plays every wave and every lane, in the order `reverse` selects; the LDS blocks are exactly as large as
 * the kernels declare them and filled with 0xA5 before every wave.  What the view owns is allocated exactly — `pre` ends at pre[n_visible] of the last good log —
 * and a query is given NOTHING of the batch's values or of the string table: the view keeps the span rows of the result and a copy of the range's log_off.
 */
#include "emu_text.cc"

#include "../../peritext_amd/csrc/view_core.h"

extern "C" uint32_t ptx_emu_view_find_step(void) { return PTX_FIND_STEP; }
extern "C" uint32_t ptx_emu_view_slice_block(void) { return PTX_SLICE_BLOCK; }

static void emu_view_scan2(uint64_t* off, uint64_t n) { /* ptx_text_offsets_kernel: two rows [2][n + 1], counts in, exclusive prefix sums out */
    for (uint32_t k = 0; k < 2; ++k) {
        uint64_t* row = off + (uint64_t)k * (n + 1);
        uint64_t run = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t v = row[i];
            row[i] = run;
            run += v;
        }
        row[n] = run;
    }
}

struct EmuView {
    const ptx_span* spans;      /* the result's */
    uint32_t first_log, n_logs;
    uint32_t* status;
    uint64_t *off, *pre_off, *log_off, *every_log;
    uint16_t* text;
    uint32_t *span_unit, *pre;
    uint64_t n_units, n_spans, n_pre;
};

static void* emu_view_block(size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (p) memset(p, 0xA5, bytes ? bytes : 1);
    return p;
}

extern "C" void ptx_emu_view_close(EmuView* v) {
    if (!v) return;
    free(v->status), free(v->off), free(v->pre_off), free(v->log_off), free(v->every_log), free(v->text), free(v->span_unit), free(v->pre);
    delete v;
}

/* ptx_text_view_create over host arrays.  Returns 0 and a handle, PTX_ERR_INVALID_ARG as the library would (a range outside the batch), or -1. */
extern "C" int ptx_emu_view_create(const uint64_t* log_off, uint32_t batch_logs, const ptx_log_result* logs, const uint32_t* values, const ptx_span* spans, const uint16_t* units,
                                   const uint64_t* str_off, uint32_t n_strings, uint32_t first_log, uint32_t n_logs, int reverse, EmuView** out) {
    *out = nullptr;
    if ((uint64_t)first_log + n_logs > batch_logs) return PTX_ERR_INVALID_ARG;
    EmuView* v = new EmuView();
    memset(v, 0, sizeof(*v));
    v->spans = spans;
    v->first_log = first_log;
    v->n_logs = n_logs;
    *out = v;
    if (n_logs == 0) return 0;
    const size_t no = (size_t)n_logs + 1;
    v->status = (uint32_t*)emu_view_block((size_t)n_logs * 4);
    v->off = (uint64_t*)emu_view_block(2 * no * 8);
    v->pre_off = (uint64_t*)emu_view_block(2 * no * 8);
    v->log_off = (uint64_t*)emu_view_block(no * 8);
    v->every_log = (uint64_t*)emu_view_block(no * 8);
    if (!v->status || !v->off || !v->pre_off || !v->log_off || !v->every_log) return -1;
    memcpy(v->log_off, log_off + first_log, no * 8);
    int rc = ptx_emu_text_lengths(log_off, batch_logs, logs, values, spans, units, str_off, n_strings, first_log, n_logs, reverse, v->status, v->off);
    if (rc != 0) return rc;
    PtxSliceArgs A;
    memset(&A, 0, sizeof(A));
    A.T.log_off = log_off;
    A.T.logs = logs;
    A.T.values = values;
    A.T.spans = spans;
    A.T.units = units;
    A.T.str_off = str_off;
    A.T.n_strings = n_strings;
    A.T.first_log = first_log;
    A.T.n_logs = n_logs;
    A.T.status = v->status;
    A.T.off = v->off;
    A.slice_off = v->every_log;
    A.n_slices = n_logs;
    A.pre_off = v->pre_off;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < n_logs; ++i) ptx_view_plan_one(A, v->every_log, ptx_emu_ix(i, n_logs));
    emu_view_scan2(v->pre_off, n_logs);
    v->n_units = v->off[n_logs];
    v->n_spans = v->off[no + n_logs];
    v->n_pre = v->pre_off[n_logs];
    v->text = (uint16_t*)emu_view_block((size_t)v->n_units * 2);
    v->span_unit = (uint32_t*)emu_view_block((size_t)v->n_spans * 4);
    v->pre = (uint32_t*)emu_view_block((size_t)v->n_pre * 4);
    if (!v->text || !v->span_unit || !v->pre) return -1;
    rc = ptx_emu_text_assemble(log_off, logs, values, spans, units, str_off, n_strings, first_log, n_logs, reverse, v->status, v->off, v->text, v->span_unit);
    if (rc != 0) return rc;
    A.T.text = v->text;
    A.T.span_unit = v->span_unit;
    A.pre = v->pre;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_SLICE_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < n_logs; ++l) {
        memset(lds, 0xA5, PTX_SLICE_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_slice_prefix_log<0>(A, l, lds);
    }
    free(lds);
    return 0;
}

/* sizes: n_units, n_spans, n_pre (ptx_view_info) */
extern "C" void ptx_emu_view_sizes(const EmuView* v, uint64_t* out) { out[0] = v->n_units, out[1] = v->n_spans, out[2] = v->n_pre; }

/* what the view holds, copied out: status [n_logs], off [2][n_logs + 1], text, span_unit, pre_off [n_logs + 1], pre */
extern "C" void ptx_emu_view_read(const EmuView* v, uint32_t* status, uint64_t* off, uint16_t* text, uint32_t* span_unit, uint64_t* pre_off, uint32_t* pre) {
    if (v->n_logs == 0) {
        off[0] = off[1] = pre_off[0] = 0;
        return;
    }
    const size_t no = (size_t)v->n_logs + 1;
    memcpy(status, v->status, (size_t)v->n_logs * 4);
    memcpy(off, v->off, 2 * no * 8);
    memcpy(text, v->text, (size_t)v->n_units * 2);
    memcpy(span_unit, v->span_unit, (size_t)v->n_spans * 4);
    memcpy(pre_off, v->pre_off, no * 8);
    memcpy(pre, v->pre, (size_t)v->n_pre * 4);
}

/* the host library's view_text_args: the range rebased to log 0 of the view's own log_off; no values, no string table */
static void emu_view_text_args(const EmuView* v, PtxTextArgs& T) {
    memset(&T, 0, sizeof(T));
    T.log_off = v->log_off;
    T.logs = nullptr; /* n_visible comes from the view's prefix */
    T.spans = v->spans;
    T.first_log = 0;
    T.n_logs = v->n_logs;
    T.status = v->status;
    T.off = v->off;
    T.text = v->text;
    T.span_unit = v->span_unit;
}

static void emu_view_find_args(const EmuView* v, PtxViewArgs& V, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t cap) {
    memset(&V, 0, sizeof(V));
    emu_view_text_args(v, V.F.T);
    V.F.pattern = pattern;
    V.F.n_pattern = n_pattern;
    V.F.flags = flags;
    V.F.cap = cap;
    V.pre_off = v->pre_off;
    V.pre = v->pre;
}

/* the count pass and the scan: n_matches [n_logs], hit_off [n_logs + 1].  Returns 0, PTX_ERR_INVALID_ARG as the library would, or -1. */
extern "C" int ptx_emu_view_count(const EmuView* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t cap, int reverse, uint32_t* n_matches, uint64_t* hit_off) {
    if (!v) return PTX_ERR_INVALID_ARG;
    if (!pattern || n_pattern == 0 || n_pattern > PTX_FIND_PATTERN_MAX || (flags & ~PTX_FIND_ASCII_NOCASE)) return PTX_ERR_INVALID_ARG;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_FIND_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    PtxViewArgs V;
    emu_view_find_args(v, V, pattern, n_pattern, flags, cap);
    V.F.n_matches = n_matches;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < v->n_logs; ++l) {
        memset(lds, 0xA5, PTX_FIND_LDS_BYTES);
        ptx_find_count_log<0>(V.F, l, lds);
    }
    uint64_t run = 0;
    for (uint32_t l = 0; l < v->n_logs; ++l) {
        hit_off[l] = run;
        run += n_matches[l] < cap ? n_matches[l] : cap;
    }
    hit_off[v->n_logs] = run;
    free(lds);
    return 0;
}

/* positions, locate and — with win_start — windows: hit_unit / hit_start / hit_end and win_start / win_end / match_unit: [hit_off[n_logs]], the caller's */
extern "C" int ptx_emu_view_hits(const EmuView* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t cap, int reverse, const uint64_t* hit_off, uint32_t* hit_unit,
                                 uint32_t* hit_start, uint32_t* hit_end, uint32_t before, uint32_t after, uint32_t* win_start, uint32_t* win_end, uint32_t* match_unit) {
    const uint64_t nh = hit_off[v->n_logs];
    if (nh == 0) return 0;
    if (nh > 0xFFFFFFFFull) return PTX_ERR_CAPACITY;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_FIND_LDS_PRE + 63u) & ~63u); /* ptx_view_positions_kernel declares no more */
    if (!lds) return -1;
    PtxViewArgs V;
    emu_view_find_args(v, V, pattern, n_pattern, flags, cap);
    V.F.hit_off = (uint64_t*)hit_off;
    V.F.hit_unit = hit_unit;
    V.F.hit_start = hit_start;
    V.F.hit_end = hit_end;
    V.n_hits = (uint32_t)nh;
    V.before = before;
    V.after = after;
    V.win_start = win_start;
    V.win_end = win_end;
    V.match_unit = match_unit;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < v->n_logs; ++l) {
        memset(lds, 0xA5, PTX_FIND_LDS_PRE);
        (void)ptx_find_positions_log<0>(V.F, l, lds);
    }
    free(lds);
    for (uint32_t i = 0; i < V.n_hits; ++i) ptx_view_locate_one(V, ptx_emu_ix(i, V.n_hits));
    if (win_start)
        for (uint32_t i = 0; i < V.n_hits; ++i) ptx_view_windows_one(V, ptx_emu_ix(i, V.n_hits));
    return 0;
}

struct EmuViewCut {
    PtxSliceArgs A;
    uint32_t *slice_log, *first_span;
    uint64_t* src_off;
    uint8_t* lds;
};

extern "C" void ptx_emu_view_cut_close(EmuViewCut* s) {
    if (!s) return;
    free(s->slice_log), free(s->first_span), free(s->src_off), free(s->lds);
    delete s;
}

/* Bounds and the scan over the view's prefix.  check != 0: the three arrays are a caller's (ptx_view_text_slices' argument checks apply); 0: they are the hits' and
 * the windows pass's.  elem_start / elem_end: [n_slices]; out_off: [2][n_slices + 1]. */
extern "C" int ptx_emu_view_bounds(const EmuView* v, const uint64_t* slice_off, const uint32_t* slice_start, const uint32_t* slice_end, int check, int reverse, uint32_t* elem_start,
                                   uint32_t* elem_end, uint64_t* out_off, EmuViewCut** handle) {
    *handle = nullptr;
    if (!v) return PTX_ERR_INVALID_ARG;
    const uint32_t n_logs = v->n_logs;
    if (check) {
        if (n_logs && (!slice_off || slice_off[0] != 0)) return PTX_ERR_INVALID_ARG;
        for (uint32_t l = 0; l < n_logs; ++l)
            if (slice_off[l + 1] < slice_off[l]) return PTX_ERR_INVALID_ARG;
    }
    const uint64_t ns64 = n_logs ? slice_off[n_logs] : 0;
    if (ns64 > 0xFFFFFFFFull || (ns64 && (!slice_start || !slice_end))) return PTX_ERR_INVALID_ARG;
    const uint32_t ns = (uint32_t)ns64;
    out_off[0] = out_off[ns64 + 1] = 0;
    EmuViewCut* s = new EmuViewCut();
    memset(s, 0, sizeof(*s));
    *handle = s;
    if (ns == 0) return 0;
    PtxSliceArgs& A = s->A;
    emu_view_text_args(v, A.T);
    A.slice_off = slice_off;
    A.slice_start = slice_start;
    A.slice_end = slice_end;
    A.n_slices = ns;
    A.pre_off = v->pre_off;
    A.pre = v->pre;
    A.elem_start = elem_start;
    A.elem_end = elem_end;
    A.out_off = out_off;
    s->lds = (uint8_t*)aligned_alloc(64, (PTX_SLICE_LDS_BYTES + 63u) & ~63u);
    A.slice_log = s->slice_log = (uint32_t*)emu_view_block((size_t)ns * 4);
    A.first_span = s->first_span = (uint32_t*)emu_view_block((size_t)ns * 4);
    A.src_off = s->src_off = (uint64_t*)emu_view_block((size_t)ns * 8);
    if (!s->lds || !s->slice_log || !s->first_span || !s->src_off) return -1;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < ns; ++i) ptx_slice_bounds_one(A, ptx_emu_ix(i, ns));
    emu_view_scan2(out_off, ns);
    return 0;
}

/* The copy and span passes: out_text: [unit_off[n_slices]], out_spans / out_span_unit: [sspan_off[n_slices]], the caller's. */
extern "C" int ptx_emu_view_emit(EmuViewCut* s, int reverse, uint16_t* out_text, ptx_span* out_spans, uint32_t* out_span_unit) {
    PtxSliceArgs& A = s->A;
    const uint32_t ns = A.n_slices;
    if (ns == 0) return 0;
    A.out_text = out_text;
    A.out_spans = out_spans;
    A.out_span_unit = out_span_unit;
    ptx_emu_reverse = reverse;
    const uint64_t units = A.out_off[ns], rows = A.out_off[(uint64_t)ns + 1u + ns];
    const uint32_t blocks = (uint32_t)((units + PTX_SLICE_BLOCK - 1u) / PTX_SLICE_BLOCK);
    for (uint32_t i = 0; i < blocks; ++i) {
        memset(s->lds, 0xA5, PTX_SLICE_LDS_BYTES);
        ptx_slice_copy_block<0>(A, ptx_emu_ix(i, blocks), s->lds);
    }
    for (uint64_t r = 0; r < rows; ++r) ptx_slice_span_one(A, reverse == 1 ? rows - 1u - r : r);
    return 0;
}
