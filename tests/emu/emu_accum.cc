/*
 * Host emulation of the accumulation of patch streams (peritext_amd/csrc/accum_core.h) — TEST TOOLING ONLY, like emu_driver.cc.
 *
 * Built into tests/emu/libperitext_emu_accum.so by __graft_entry__.build() and loaded only by tests/test_emu_accum.py; tests/emu/emu_accum_main.cc includes
 * this file into a stand-alone sanitizer program.  One host thread plays the wave of every log in the lane order `reverse` selects.  A log goes through the LDS
 * store when its state fits `lds_bytes` and hbm == 0, through the HBM store otherwise — the routing of the host library.  The LDS block (exactly what the log
 * needs) and the state slice (exactly its units) are filled with 0xA5 first: the kernel zeroes what it needs zeroed.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
PTX_DEV uint32_t ptx_l2_load32(const uint32_t* p) { return *p; } /* (ptx_platform_gfx950.h: a device-scope load; the emulation has one memory) */
#include "../../peritext_amd/csrc/accum_core.h"

/* What ptx_accumulate_patches (want == NULL) / the tail of ptx_check_patches (want, check set) do, over a host batch.  res: [n_logs]; values / spans / cints: one
 * row per op row of the batch, or all NULL.  used_hbm (optional): [n_logs], 1 where the log took the HBM store.  Returns 0, or -1 (out of memory). */
extern "C" int ptx_emu_accum(const ptx_batch* b, const uint64_t* patch_off, const ptx_patch_log* plogs, const ptx_patch* patches, ptx_log_result* res, uint32_t* values,
                             ptx_span* spans, ptx_cinterval* cints, const ptx_log_result* want, ptx_patch_check_log* check, int hbm, int reverse, uint32_t lds_bytes,
                             uint8_t* used_hbm) {
    const uint32_t L = b->n_logs;
    ptx_log_hdr* hdr = (ptx_log_hdr*)calloc(L ? L : 1, sizeof(ptx_log_hdr));
    if (!hdr) return -1;
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t b0 = b->log_off[l], b1 = b->log_off[l + 1];
        if (b->log_hdr) hdr[l] = b->log_hdr[l];
        else ptx_census_rows(b->op_id + b0, b->action + b0, b->mark_type + b0, b->payload + b0, b1 - b0, &hdr[l]);
    }
    PtxAccumArgs A;
    memset(&A, 0, sizeof(A));
    A.log_off = b->log_off;
    A.payload = b->payload;
    A.action = b->action;
    A.mark_type = b->mark_type;
    A.log_hdr = hdr;
    A.patches = patches;
    A.rec_off = patch_off;
    A.rec_base = 0;
    A.plogs = plogs;
    A.res = res;
    A.out_values = values;
    A.out_spans = spans;
    A.out_cints = cints;
    A.want = want;
    A.check = check;
    A.n_launch = 1;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t rows = b->log_off[l + 1] - b->log_off[l], need = ptx_accum_lds_need_hdr(rows, hdr[l]), units = ptx_accum_units_hdr(rows, hdr[l]);
        const bool to_hbm = hbm || need > lds_bytes;
        if (used_hbm) used_hbm[l] = to_hbm ? 1 : 0;
        A.first_log = l;
        if (to_hbm) {
            uint64_t soff[2] = {0, units};
            uint32_t* state = (uint32_t*)malloc(units * 4 + 4);
            uint8_t* lds = (uint8_t*)malloc(PTX_ACCUM_HBM_LDS_BYTES);
            if (!state || !lds) {
                free(state);
                free(lds);
                free(hdr);
                return -1;
            }
            memset(state, 0xA5, units * 4);
            memset(lds, 0xA5, PTX_ACCUM_HBM_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
            A.state = state;
            A.state_off = soff;
            ptx_accum_log_hbm<0>(A, 0, lds);
            free(lds);
            free(state);
        } else {
            uint8_t* lds = (uint8_t*)malloc(need);
            if (!lds) {
                free(hdr);
                return -1;
            }
            memset(lds, 0xA5, need);
            A.state = nullptr;
            A.state_off = nullptr;
            A.lds_bytes = (uint32_t)need;
            ptx_accum_log<0>(A, 0, lds);
            free(lds);
        }
    }
    free(hdr);
    return 0;
}
extern "C" uint64_t ptx_emu_accum_lds_need(uint64_t rows, uint32_t n_ins, uint32_t n_comment_ids) {
    ptx_log_hdr h;
    memset(&h, 0, sizeof(h));
    h.n_ins = n_ins;
    h.n_comment_ids = n_comment_ids;
    return ptx_accum_lds_need_hdr(rows, h);
}
