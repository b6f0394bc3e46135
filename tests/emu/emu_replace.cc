/*
 * Host emulation of find and replace on a view (peritext_amd/csrc/replace_core.h) — TEST TOOLING ONLY, like emu_view.cc.
 *
 * Built into tests/emu/libperitext_emu_replace.so by __graft_entry__.build() and loaded only by tests/test_emu_replace.py; tests/emu/emu_replace_main.cc includes
 * this file into a stand-alone sanitizer program.  The passes take what the view's own passes leave — the view's status and element prefix, and the hits of
 * ptx_find_count_log / ptx_find_positions_log / ptx_view_locate_one with no cap, which tests/test_emu_view.py's emulation makes — and are played the way
 * view_replace_impl launches them: select (a wave per log), the two scans (the host library's ptx_find_offsets_kernel, here a plain loop), emit (a lane per
 * hit).  One host thread plays every wave and every lane, in the order `reverse` selects; the LDS block is exactly PTX_REPLACE_LDS_BYTES and filled with 0xA5
 * before every wave.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
#include "../../peritext_amd/csrc/replace_core.h"

extern "C" uint32_t ptx_emu_replace_tile(void) { return PTX_REPLACE_TILE; }
extern "C" uint32_t ptx_emu_replace_rows_max(void) { return PTX_CHANGE_ROWS_MAX; }

/* the argument checks of ptx_view_replace_plan: 0 or PTX_ERR_INVALID_ARG */
extern "C" int ptx_emu_replace_check(int has_view, int has_pattern, uint32_t n_pattern, uint32_t flags, int has_replacement, uint32_t n_replacement, uint32_t first_log, uint32_t n_logs,
                                     uint32_t n_batch_logs) {
    if (!has_view) return PTX_ERR_INVALID_ARG;
    if (!has_pattern || n_pattern == 0 || n_pattern > PTX_FIND_PATTERN_MAX || (flags & ~PTX_FIND_ASCII_NOCASE)) return PTX_ERR_INVALID_ARG;
    if (n_replacement > PTX_CHANGE_ROWS_MAX || (n_replacement && !has_replacement)) return PTX_ERR_INVALID_ARG;
    if ((uint64_t)n_batch_logs < (uint64_t)first_log + n_logs) return PTX_ERR_INVALID_ARG;
    return 0;
}

struct EmuReplaceIn {
    const uint32_t* status;   /* the view's [n_logs] */
    const uint64_t* pre_off;  /* ... [n_logs + 1] */
    const uint32_t* pre;
    const uint64_t* hit_off;  /* [n_logs + 1], no cap */
    const uint32_t* hit_unit;
    const uint32_t* hit_start;
    const uint32_t* hit_end;
    uint32_t n_logs, n_pattern, n_replacement, first_log, n_batch_logs;
};

static void emu_replace_args(const EmuReplaceIn* in, PtxReplaceArgs& R) {
    memset(&R, 0, sizeof(R));
    R.V.F.T.n_logs = in->n_logs;
    R.V.F.T.status = (uint32_t*)in->status;
    R.V.F.hit_off = (uint64_t*)in->hit_off;
    R.V.F.hit_unit = (uint32_t*)in->hit_unit;
    R.V.F.hit_start = (uint32_t*)in->hit_start;
    R.V.F.hit_end = (uint32_t*)in->hit_end;
    R.V.F.n_pattern = in->n_pattern;
    R.V.pre_off = in->pre_off;
    R.V.pre = in->pre;
    R.V.n_hits = (uint32_t)in->hit_off[in->n_logs];
    R.n_replacement = in->n_replacement;
    R.first_log = in->first_log;
    R.n_batch_logs = in->n_batch_logs;
}

static void emu_replace_scan(const uint32_t* v, uint64_t* off, uint32_t n) { /* ptx_find_offsets_kernel with cap 0xFFFFFFFF */
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; ++i) {
        off[i] = run;
        run += v[i];
    }
    off[n] = run;
}

/* select and the two scans.  sel: [n_hits]; status, n_chosen, n_replaced, n_ops: [n_logs]; makes: [n_batch_logs]; chg_off: [n_batch_logs + 1]; op_log_off: [n_logs + 1].
 * A view without hits is the library's all-zero plan: no pass runs.  Returns 0, PTX_ERR_CAPACITY for more than 2^32 - 1 hits, or -1. */
extern "C" int ptx_emu_replace_select(const EmuReplaceIn* in, int reverse, uint32_t* sel, uint32_t* status, uint32_t* n_chosen, uint32_t* n_replaced, uint32_t* n_ops, uint32_t* makes,
                                      uint64_t* chg_off, uint64_t* op_log_off) {
    const uint32_t n_logs = in->n_logs;
    const uint64_t nh = n_logs ? in->hit_off[n_logs] : 0;
    if (nh > 0xFFFFFFFFull) return PTX_ERR_CAPACITY;
    if (nh == 0) {
        for (uint32_t l = 0; l < n_logs; ++l) status[l] = in->status[l], n_chosen[l] = n_replaced[l] = n_ops[l] = 0;
        for (uint32_t b = 0; b < in->n_batch_logs; ++b) makes[b] = 0;
        for (uint64_t b = 0; b <= in->n_batch_logs; ++b) chg_off[b] = 0;
        for (uint32_t l = 0; l <= n_logs; ++l) op_log_off[l] = 0;
        return 0;
    }
    PtxReplaceArgs R;
    emu_replace_args(in, R);
    R.sel = sel;
    R.status = status;
    R.n_chosen = n_chosen;
    R.n_replaced = n_replaced;
    R.n_ops = n_ops;
    R.makes = makes;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (PTX_REPLACE_LDS_BYTES + 63u) & ~63u);
    if (!lds) return -1;
    memset(makes, 0, (size_t)in->n_batch_logs * 4); /* the library's hipMemsetAsync */
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < n_logs; ++i) {
        memset(lds, 0xA5, PTX_REPLACE_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_replace_select_log<0>(R, ptx_emu_ix(i, n_logs), lds);
    }
    free(lds);
    emu_replace_scan(makes, chg_off, in->n_batch_logs);
    emu_replace_scan(n_ops, op_log_off, n_logs);
    return 0;
}

/* emit: op_off: [n_changes + 1]; the five columns: [n_input_ops] = op_log_off[n_logs].  No ops: nothing runs and op_off = {0}, as the library's. */
extern "C" int ptx_emu_replace_emit(const EmuReplaceIn* in, int reverse, const uint32_t* sel, const uint32_t* n_replaced, const uint32_t* n_ops, const uint64_t* chg_off,
                                    const uint64_t* op_log_off, uint64_t* op_off, uint8_t* action, uint8_t* mark_type, uint32_t* index, uint32_t* count, uint32_t* payload) {
    if (in->n_logs == 0 || op_log_off[in->n_logs] == 0) {
        op_off[0] = 0;
        return 0;
    }
    PtxReplaceArgs R;
    emu_replace_args(in, R);
    R.sel = (uint32_t*)sel;
    R.n_replaced = (uint32_t*)n_replaced;
    R.n_ops = (uint32_t*)n_ops;
    R.chg_off = (uint64_t*)chg_off;
    R.op_log_off = (uint64_t*)op_log_off;
    R.op_off = op_off;
    R.action = action;
    R.mark_type = mark_type;
    R.index = index;
    R.count = count;
    R.payload = payload;
    ptx_emu_reverse = reverse;
    for (uint32_t i = 0; i < R.V.n_hits; ++i) ptx_replace_emit_one(R, ptx_emu_ix(i, R.V.n_hits));
    return 0;
}
