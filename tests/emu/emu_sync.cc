/*
 * Host emulation of the sync of replica logs (peritext_amd/csrc/sync_core.h) — TEST TOOLING ONLY, like emu_driver.cc.
 *
 * Built into tests/emu/libperitext_emu_sync.so by __graft_entry__.build() and loaded only by tests/test_emu_sync.py; tests/emu/emu_sync_main.cc includes
 * this file into a stand-alone sanitizer program.  One host thread plays the plan wave and the gather workgroup of every pair, in the lane order `reverse`
 * selects; the LDS block is exactly what the host library asks for and, like the scratch, filled with 0xA5 first: the kernel zeroes what it needs zeroed.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
#include "../../peritext_amd/csrc/sync_core.h"

/* What ptx_sync_replicas does with a resident batch, over a host one.  status / n_admitted / n_rows: [n_pairs].  The columns of `more` are the caller's, sized for
 * the worst case (every row / change of every pair's source log); o_log_off / o_chg_off: [n_logs + 1].  Returns 0, PTX_ERR_INVALID_ARG as the library would, or
 * -1 (out of memory). */
extern "C" int ptx_emu_sync(const ptx_batch* b, uint32_t n_pairs, const uint32_t* src_log, const uint32_t* dst_log, uint32_t max_attempts, int reverse, uint32_t* status,
                            uint32_t* n_admitted, uint32_t* n_rows, uint64_t* o_log_off, uint64_t* o_chg_off, uint64_t* o_op_id, uint64_t* o_ref_a, uint64_t* o_ref_b,
                            uint32_t* o_payload, uint8_t* o_action, uint8_t* o_mark_type, uint8_t* o_side_a, uint8_t* o_side_b, uint32_t* o_chg_hdr, uint16_t* o_chg_env,
                            uint16_t* o_chg_env_hi) {
    const uint32_t L = b->n_logs, P = n_pairs;
    if (!b->chg_off || !b->chg_hdr || !b->chg_env || b->max_actors == 0) return PTX_ERR_INVALID_ARG;
    uint8_t* seen = (uint8_t*)malloc(L ? L : 1);
    if (!seen) return -1;
    const int bad = ptx_sync_check_pairs(L, P, src_log, dst_log, seen);
    free(seen);
    if (bad) return PTX_ERR_INVALID_ARG;
    uint64_t* scr = (uint64_t*)calloc((size_t)P + 1, 8);
    if (!scr) return -1;
    for (uint32_t p = 0; p < P; ++p) scr[p + 1] = scr[p] + ptx_sync_scratch_words(b->chg_off[src_log[p] + 1] - b->chg_off[src_log[p]]);
    const size_t lds_bytes = (size_t)ptx_sync_lds_need(b->max_actors);
    uint32_t* scratch = (uint32_t*)malloc(scr[P] * 4 + 4);
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (lds_bytes + 63) & ~(size_t)63);
    if (!scratch || !lds) return -1;
    memset(scratch, 0xA5, scr[P] * 4);
    PtxSyncArgs A;
    memset(&A, 0, sizeof(A));
    A.log_off = b->log_off;
    A.chg_off = b->chg_off;
    A.chg_hdr = b->chg_hdr;
    A.chg_env = b->chg_env;
    A.chg_env_hi = b->chg_env_hi;
    A.max_actors = b->max_actors;
    A.n_pairs = P;
    A.max_attempts = max_attempts;
    A.src_log = src_log;
    A.dst_log = dst_log;
    A.scr_off = scr;
    A.scratch = scratch;
    A.status = status;
    A.n_admitted = n_admitted;
    A.n_rows = n_rows;
    A.lds_bytes = (uint32_t)lds_bytes;
    ptx_emu_reverse = reverse;
    for (uint32_t p = 0; p < P; ++p) {
        memset(lds, 0xA5, lds_bytes); /* LDS is not zero-initialised on the GPU either */
        ptx_sync_plan_pair<0>(A, p, lds);
#if defined(__SANITIZE_ADDRESS__)
        ASAN_UNPOISON_MEMORY_REGION(lds, lds_bytes); /* (the bump allocator's padding marks of this pair) */
#endif
    }
    for (uint32_t l = 0; l <= L; ++l) o_log_off[l] = o_chg_off[l] = 0;
    for (uint32_t p = 0; p < P; ++p) {
        o_chg_off[dst_log[p] + 1] = n_admitted[p];
        o_log_off[dst_log[p] + 1] = n_rows[p];
    }
    for (uint32_t l = 0; l < L; ++l) {
        o_log_off[l + 1] += o_log_off[l];
        o_chg_off[l + 1] += o_chg_off[l];
    }
    PtxSyncGatherArgs G = {b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b, o_op_id, o_ref_a, o_ref_b, o_payload, o_action, o_mark_type,
                           o_side_a, o_side_b, o_chg_hdr, o_chg_env, b->chg_env_hi ? o_chg_env_hi : nullptr, o_log_off, o_chg_off};
    for (uint32_t p = 0; p < P; ++p) ptx_sync_gather_pair<0>(A, G, p);
    free(lds);
    free(scratch);
    free(scr);
    return 0;
}
