/*
 * Host emulation of the preparation of change() from resident InputOperations (peritext_amd/csrc/change_prep_core.h) — TEST TOOLING ONLY, like emu_replace.cc.
 *
 * Built into tests/emu/libperitext_emu_change_prep.so by __graft_entry__.build() and loaded only by the tests of change_prep_cases.py;
 * tests/emu/emu_change_prep_main.cc includes this file into a stand-alone sanitizer program.  The passes are played the way ptx_change_device launches them: the
 * offsets check (a lane per entry of chg_off and of op_off), the prepare pass (a wave per log), and the two scans (the host library's ptx_find_offsets_kernel,
 * here a plain loop as in emu_replace.cc).  One host thread plays every wave and every lane, in the order `reverse` selects; the LDS block is exactly
 * PTX_CHANGE_PREP_LDS_BYTES and filled with 0xA5 before every wave.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
#include "../../peritext_amd/csrc/change_prep_core.h"

extern "C" uint32_t ptx_emu_prep_abi_version(void) { return PTX_ABI_VERSION; }
extern "C" uint32_t ptx_emu_prep_rows_max(void) { return PTX_CHANGE_ROWS_MAX; }
extern "C" uint32_t ptx_emu_prep_log_hdr_bytes(void) { return (uint32_t)sizeof(ptx_log_hdr); }
/* the two helpers of change_core.h as ptx_change calls them on the host: what the tests expect the device to have computed */
extern "C" uint64_t ptx_emu_change_lds_need(uint64_t n, uint64_t grow, uint64_t ks, uint64_t na, int list_in_hbm) { return ptx_change_lds_need(n, grow, ks, na, list_in_hbm != 0); }
extern "C" uint64_t ptx_emu_change_list_words(uint64_t n, uint64_t grow) { return ptx_change_list_words(n, grow); }

struct EmuPrepIn {
    const uint64_t* chg_off;
    const uint64_t* op_off;
    const uint8_t* action;
    const uint32_t* count;
    const uint32_t* payload;
    uint64_t n_changes, n_input_ops, n_values;
    uint32_t has_values, n_logs;
    const uint64_t* log_off;
    const void* log_hdr; /* ptx_log_hdr [n_logs] */
    uint32_t max_actors, all_in_hbm;
    uint64_t max_lds;
};

static void emu_prep_scan(const uint32_t* v, uint64_t* off, uint32_t n) { /* ptx_find_offsets_kernel with cap 0xFFFFFFFF */
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; ++i) {
        off[i] = run;
        run += v[i];
    }
    off[n] = run;
}

/* rows, list_words: [n_logs]; out_off, list_off: [n_logs + 1]; err, lds_need: one word each.  The scans run whatever the verdict, as the library's do. */
extern "C" int ptx_emu_change_prep(const EmuPrepIn* in, int reverse, uint32_t* rows, uint32_t* list_words, uint64_t* out_off, uint64_t* list_off, uint64_t* err, uint64_t* lds_need) {
    PtxChangePrepArgs A;
    memset(&A, 0, sizeof(A));
    A.chg_off = in->chg_off;
    A.op_off = in->op_off;
    A.action = in->action;
    A.count = in->count;
    A.payload = in->payload;
    A.n_changes = in->n_changes;
    A.n_input_ops = in->n_input_ops;
    A.n_values = in->n_values;
    A.has_values = in->has_values;
    A.n_logs = in->n_logs;
    A.log_off = in->log_off;
    A.log_hdr = (const ptx_log_hdr*)in->log_hdr;
    A.max_actors = in->max_actors;
    A.all_in_hbm = in->all_in_hbm;
    A.max_lds = in->max_lds;
    A.rows = rows;
    A.list_words = list_words;
    unsigned long long e = PTX_CP_NO_ERROR, need = 0; /* the library's two memsets */
    A.err = &e;
    A.lds_need = &need;
    ptx_emu_reverse = reverse;
    const uint64_t entries = ptx_change_offsets_entries(A);
    if (entries > 0xFFFFFFFFull) return -1;
    for (uint32_t k = 0; k < (uint32_t)entries; ++k) ptx_change_offsets_check_one(A, ptx_emu_ix(k, (uint32_t)entries));
    uint8_t* lds = (uint8_t*)aligned_alloc(64, 64);
    if (!lds) return -1;
    for (uint32_t k = 0; k < in->n_logs; ++k) {
        memset(lds, 0xA5, PTX_CHANGE_PREP_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_change_prep_log<0>(A, ptx_emu_ix(k, in->n_logs), lds);
    }
    free(lds);
    emu_prep_scan(rows, out_off, in->n_logs);
    emu_prep_scan(list_words, list_off, in->n_logs);
    *err = e;
    *lds_need = need;
    return 0;
}
