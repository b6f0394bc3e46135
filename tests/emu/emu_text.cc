/*
 * Host emulation of the document-text passes (peritext_amd/csrc/text_core.h) — TEST TOOLING ONLY, like emu_versions.cc.
 *
 * Built into tests/emu/libperitext_emu_text.so by __graft_entry__.build() and loaded only by tests/test_emu_text.py; tests/emu/emu_text_main.cc includes this
 * file into a stand-alone sanitizer program.  One host thread plays the wave of every log, in the lane order `reverse` selects; the LDS block is exactly
 * PTX_TEXT_LDS_BYTES and filled with 0xA5 before every log: the kernels initialise what they read.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
#include "../../peritext_amd/csrc/text_core.h"

extern "C" uint32_t ptx_emu_text_tile(void) { return PTX_TEXT_TILE; }
extern "C" uint32_t ptx_emu_text_lane_max(void) { return PTX_TEXT_LANE_MAX; }

/* Pass 1 of ptx_result_text_range over host arrays: the merge's result in the capacity layout (a log's values / spans at row log_off[l]), the string table as
 * ptx_strings_upload takes it.  status: [n_logs]; off: [2][n_logs + 1], on return the exclusive prefix sums text_off | span_off (the host library's scan kernel,
 * here a plain loop).  Returns 0, PTX_ERR_INVALID_ARG as the library would (a range outside the batch, offsets that are no string table), or -1. */
extern "C" int ptx_emu_text_lengths(const uint64_t* log_off, uint32_t batch_logs, const ptx_log_result* logs, const uint32_t* values, const ptx_span* spans, const uint16_t* units,
                                    const uint64_t* str_off, uint32_t n_strings, uint32_t first_log, uint32_t n_logs, int reverse, uint32_t* status, uint64_t* off) {
    if ((uint64_t)first_log + n_logs > batch_logs) return PTX_ERR_INVALID_ARG;
    if (str_off[0] != 0) return PTX_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_strings; ++i)
        if (str_off[i + 1] < str_off[i]) return PTX_ERR_INVALID_ARG;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_TEXT_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    PtxTextArgs A;
    memset(&A, 0, sizeof(A));
    A.log_off = log_off;
    A.logs = logs;
    A.values = values;
    A.spans = spans;
    A.units = units;
    A.str_off = str_off;
    A.n_strings = n_strings;
    A.first_log = first_log;
    A.n_logs = n_logs;
    A.status = status;
    A.off = off;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < n_logs; ++l) {
        memset(lds, 0xA5, PTX_TEXT_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_text_length_log<0>(A, l, lds);
    }
    for (uint32_t k = 0; k < 2; ++k) {
        uint64_t* row = off + (uint64_t)k * (n_logs + 1);
        uint64_t run = 0;
        for (uint32_t l = 0; l < n_logs; ++l) {
            const uint64_t v = row[l];
            row[l] = run;
            run += v;
        }
        row[n_logs] = run;
    }
    free(lds);
    return 0;
}

/* Pass 2: status / off as pass 1 left them; text: [off[0][n_logs]] (the first unit dword-aligned), span_unit: [off[1][n_logs]], both the caller's. */
extern "C" int ptx_emu_text_assemble(const uint64_t* log_off, const ptx_log_result* logs, const uint32_t* values, const ptx_span* spans, const uint16_t* units, const uint64_t* str_off,
                                     uint32_t n_strings, uint32_t first_log, uint32_t n_logs, int reverse, uint32_t* status, uint64_t* off, uint16_t* text, uint32_t* span_unit) {
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_TEXT_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    PtxTextArgs A;
    memset(&A, 0, sizeof(A));
    A.log_off = log_off;
    A.logs = logs;
    A.values = values;
    A.spans = spans;
    A.units = units;
    A.str_off = str_off;
    A.n_strings = n_strings;
    A.first_log = first_log;
    A.n_logs = n_logs;
    A.status = status;
    A.off = off;
    A.text = text;
    A.span_unit = span_unit;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < n_logs; ++l) {
        memset(lds, 0xA5, PTX_TEXT_LDS_BYTES);
        ptx_text_assemble_log<0>(A, l, lds);
    }
    free(lds);
    return 0;
}
