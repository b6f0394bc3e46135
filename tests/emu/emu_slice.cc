/*
 * Host emulation of the text and span rows of element ranges (peritext_amd/csrc/slice_core.h) — TEST TOOLING ONLY, like emu_find.cc; it includes emu_text.cc for
 * the text passes whose output the slices are cut from.
 *
 * Built into tests/emu/libperitext_emu_slice.so by __graft_entry__.build() and loaded only by tests/test_emu_slices.py; tests/emu/emu_slice_main.cc includes this
 * file into a stand-alone sanitizer program.  One host thread plays every wave and every lane, in the order `reverse` selects; the LDS block is exactly
 * PTX_SLICE_LDS_BYTES and filled with 0xA5 before every wave: the kernels initialise what they read.  The scratch blocks (the element prefixes, the three
 * per-slice columns) are exactly as large as the host library makes them.
 */
#include "emu_text.cc"

#include "../../peritext_amd/csrc/slice_core.h"

extern "C" uint32_t ptx_emu_slice_block(void) { return PTX_SLICE_BLOCK; }

static void emu_scan2(uint64_t* off, uint64_t n) { /* ptx_text_offsets_kernel: two rows [2][n + 1], counts in, exclusive prefix sums out */
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

struct EmuSlices {
    PtxSliceArgs A;
    uint64_t* pre_off;
    uint32_t* pre;
    uint32_t *slice_log, *first_span;
    uint64_t* src_off;
    uint8_t* lds;
};

extern "C" void ptx_emu_slices_close(EmuSlices* s) {
    if (!s) return;
    free(s->pre_off);
    free(s->pre);
    free(s->slice_log);
    free(s->first_span);
    free(s->src_off);
    free(s->lds);
    delete s;
}

/* Plan, prefix, bounds and the scan over what ptx_emu_text_lengths / ptx_emu_text_assemble left (status: [n_logs], off: [2][n_logs + 1], text: [off[0][n_logs]]).
 * elem_start / elem_end: [n_slices]; out_off: [2][n_slices + 1] = unit_off | sspan_off, all the caller's.  Returns 0 and a handle for ptx_emu_slices_emit,
 * PTX_ERR_INVALID_ARG as the library would, or -1. */
extern "C" int ptx_emu_slices_bounds(const uint64_t* log_off, uint32_t batch_logs, const ptx_log_result* logs, const uint32_t* values, const ptx_span* spans, const uint64_t* str_off,
                                     uint32_t n_strings, uint32_t first_log, uint32_t n_logs, const uint32_t* status, const uint64_t* off, const uint16_t* text, const uint64_t* slice_off,
                                     const uint32_t* slice_start, const uint32_t* slice_end, int reverse, uint32_t* elem_start, uint32_t* elem_end, uint64_t* out_off, EmuSlices** handle) {
    *handle = nullptr;
    if ((uint64_t)first_log + n_logs > batch_logs) return PTX_ERR_INVALID_ARG;
    if (n_logs && (!slice_off || slice_off[0] != 0)) return PTX_ERR_INVALID_ARG;
    for (uint32_t l = 0; l < n_logs; ++l)
        if (slice_off[l + 1] < slice_off[l]) return PTX_ERR_INVALID_ARG;
    const uint64_t ns64 = n_logs ? slice_off[n_logs] : 0;
    if (ns64 > 0xFFFFFFFFull || (ns64 && (!slice_start || !slice_end))) return PTX_ERR_INVALID_ARG;
    const uint32_t ns = (uint32_t)ns64;
    out_off[0] = out_off[ns64 + 1] = 0;
    EmuSlices* s = new EmuSlices();
    memset(s, 0, sizeof(*s));
    *handle = s;
    if (ns == 0) return 0;
    PtxSliceArgs& A = s->A;
    A.T.log_off = log_off;
    A.T.logs = logs;
    A.T.values = values;
    A.T.spans = spans;
    A.T.str_off = str_off;
    A.T.n_strings = n_strings;
    A.T.first_log = first_log;
    A.T.n_logs = n_logs;
    A.T.status = (uint32_t*)status;
    A.T.off = (uint64_t*)off;
    A.T.text = (uint16_t*)text;
    A.slice_off = slice_off;
    A.slice_start = slice_start;
    A.slice_end = slice_end;
    A.n_slices = ns;
    A.elem_start = elem_start;
    A.elem_end = elem_end;
    A.out_off = out_off;
    s->lds = (uint8_t*)aligned_alloc(64, (PTX_SLICE_LDS_BYTES + 63u) & ~63u);
    A.pre_off = s->pre_off = (uint64_t*)malloc(2 * ((size_t)n_logs + 1) * 8);
    A.slice_log = s->slice_log = (uint32_t*)malloc((size_t)ns * 4);
    A.first_span = s->first_span = (uint32_t*)malloc((size_t)ns * 4);
    A.src_off = s->src_off = (uint64_t*)malloc((size_t)ns * 8);
    if (!s->lds || !s->pre_off || !s->slice_log || !s->first_span || !s->src_off) return -1;
    memset(s->pre_off, 0xA5, 2 * ((size_t)n_logs + 1) * 8);
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < n_logs; ++i) ptx_slice_plan_one(A, ptx_emu_ix(i, n_logs));
    emu_scan2(s->pre_off, n_logs);
    const uint64_t words = s->pre_off[n_logs];
    A.pre = s->pre = (uint32_t*)malloc(words ? (size_t)words * 4 : 4);
    if (!s->pre) return -1;
    memset(s->pre, 0xA5, words ? (size_t)words * 4 : 4);
    for (uint32_t l = 0; l < n_logs; ++l) {
        memset(s->lds, 0xA5, PTX_SLICE_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_slice_prefix_log<0>(A, l, s->lds);
    }
    for (uint32_t i = 0; i < ns; ++i) ptx_slice_bounds_one(A, ptx_emu_ix(i, ns));
    emu_scan2(out_off, ns);
    return 0;
}

/* The copy and span passes: out_text: [unit_off[n_slices]], out_spans / out_span_unit: [sspan_off[n_slices]], the caller's. */
extern "C" int ptx_emu_slices_emit(EmuSlices* s, int reverse, uint16_t* out_text, ptx_span* out_spans, uint32_t* out_span_unit) {
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
