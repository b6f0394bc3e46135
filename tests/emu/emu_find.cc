/*
 * Host emulation of the search in the documents' text (peritext_amd/csrc/find_core.h) — TEST TOOLING ONLY, like emu_text.cc, which it includes for the text
 * passes the search reads the output of.
 *
 * Built into tests/emu/libperitext_emu_find.so by __graft_entry__.build() and loaded only by tests/test_emu_find.py; tests/emu/emu_find_main.cc includes this
 * file into a stand-alone sanitizer program.  One host thread plays the wave of every log, in the lane order `reverse` selects; the LDS block is exactly
 * PTX_FIND_LDS_BYTES and filled with 0xA5 before every log: the kernels initialise what they read.
 */
#include "emu_text.cc"

#include "../../peritext_amd/csrc/find_core.h"

extern "C" uint32_t ptx_emu_find_step(void) { return PTX_FIND_STEP; }
extern "C" uint32_t ptx_emu_find_pattern_max(void) { return PTX_FIND_PATTERN_MAX; }

static void emu_find_args(PtxFindArgs& A, const uint64_t* log_off, const ptx_log_result* logs, const uint32_t* values, const uint64_t* str_off, uint32_t n_strings, uint32_t first_log,
                          uint32_t n_logs, const uint32_t* status, const uint64_t* off, const uint16_t* text, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t cap) {
    memset(&A, 0, sizeof(A));
    A.T.log_off = log_off;
    A.T.logs = logs;
    A.T.values = values;
    A.T.str_off = str_off;
    A.T.n_strings = n_strings;
    A.T.first_log = first_log;
    A.T.n_logs = n_logs;
    A.T.status = (uint32_t*)status;
    A.T.off = (uint64_t*)off;
    A.T.text = (uint16_t*)text;
    A.pattern = pattern;
    A.n_pattern = n_pattern;
    A.flags = flags;
    A.cap = cap;
}

/* The count pass and the scan over what ptx_emu_text_lengths / ptx_emu_text_assemble left (status: [n_logs], off: [2][n_logs + 1], text: [off[0][n_logs]]).
 * n_matches: [n_logs]; hit_off: [n_logs + 1] (the host library's scan kernel, here a plain loop).  Returns 0, PTX_ERR_INVALID_ARG as the library would, or -1. */
extern "C" int ptx_emu_find_count(const uint32_t* status, const uint64_t* off, const uint16_t* text, uint32_t n_logs, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags,
                                  uint32_t cap, int reverse, uint32_t* n_matches, uint64_t* hit_off) {
    if (!pattern || n_pattern == 0 || n_pattern > PTX_FIND_PATTERN_MAX || (flags & ~PTX_FIND_ASCII_NOCASE)) return PTX_ERR_INVALID_ARG;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_FIND_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    PtxFindArgs A;
    emu_find_args(A, nullptr, nullptr, nullptr, nullptr, 0, 0, n_logs, status, off, text, pattern, n_pattern, flags, cap);
    A.n_matches = n_matches;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < n_logs; ++l) {
        memset(lds, 0xA5, PTX_FIND_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_find_count_log<0>(A, l, lds);
    }
    uint64_t run = 0;
    for (uint32_t l = 0; l < n_logs; ++l) {
        hit_off[l] = run;
        run += n_matches[l] < cap ? n_matches[l] : cap;
    }
    hit_off[n_logs] = run;
    free(lds);
    return 0;
}

/* The emit pass: hit_unit / hit_start / hit_end: [hit_off[n_logs]], the caller's. */
extern "C" int ptx_emu_find_emit(const uint64_t* log_off, const ptx_log_result* logs, const uint32_t* values, const uint64_t* str_off, uint32_t n_strings, uint32_t first_log, uint32_t n_logs,
                                 const uint32_t* status, const uint64_t* off, const uint16_t* text, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t cap, int reverse,
                                 const uint64_t* hit_off, uint32_t* hit_unit, uint32_t* hit_start, uint32_t* hit_end) {
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_FIND_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    PtxFindArgs A;
    emu_find_args(A, log_off, logs, values, str_off, n_strings, first_log, n_logs, status, off, text, pattern, n_pattern, flags, cap);
    A.hit_off = (uint64_t*)hit_off;
    A.hit_unit = hit_unit;
    A.hit_start = hit_start;
    A.hit_end = hit_end;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < n_logs; ++l) {
        memset(lds, 0xA5, PTX_FIND_LDS_BYTES);
        ptx_find_emit_log<0>(A, l, lds);
    }
    free(lds);
    return 0;
}
