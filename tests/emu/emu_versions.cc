/*
 * Host emulation of the version cuts of resident logs (peritext_amd/csrc/version_core.h) — TEST TOOLING ONLY, like emu_sync.cc.
 *
 * Built into tests/emu/libperitext_emu_versions.so by __graft_entry__.build() and loaded only by tests/test_emu_versions.py; tests/emu/emu_versions_main.cc
 * includes this file into a stand-alone sanitizer program.  One host thread plays the plan wave and the gather workgroup of every cut, in the lane order
 * `reverse` selects; the LDS block is exactly what the host library asks for and, like the scratch, filled with 0xA5 first: the kernel zeroes what it needs
 * zeroed.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
#include "../../peritext_amd/csrc/version_core.h"

/* What ptx_batch_at_versions does with a resident batch, over a host one.  status / n_kept / first_row: [n_cuts], clocks_out: [n_cuts * max_actors].  The columns
 * of the output batch are the caller's, sized for the worst case (every row / change of every cut's source log); o_log_off / o_chg_off: [n_cuts + 1].  Returns 0,
 * PTX_ERR_INVALID_ARG as the library would, or -1 (out of memory). */
extern "C" int ptx_emu_versions(const ptx_batch* b, uint32_t n_cuts, const uint32_t* src_log, const uint32_t* clocks, const uint32_t* prefix, uint32_t flags, int reverse,
                                uint32_t* status, uint32_t* n_kept, uint32_t* first_row, uint32_t* clocks_out, uint64_t* o_log_off, uint64_t* o_chg_off, uint64_t* o_op_id,
                                uint64_t* o_ref_a, uint64_t* o_ref_b, uint32_t* o_payload, uint8_t* o_action, uint8_t* o_mark_type, uint8_t* o_side_a, uint8_t* o_side_b,
                                uint32_t* o_chg_hdr, uint16_t* o_chg_env, uint16_t* o_chg_env_hi) {
    const uint32_t L = b->n_logs, P = n_cuts;
    if (!b->chg_off || !b->chg_hdr || !b->chg_env || b->max_actors == 0) return PTX_ERR_INVALID_ARG;
    if (P && (clocks != nullptr) == (prefix != nullptr)) return PTX_ERR_INVALID_ARG;
    if (flags & ~PTX_VERSIONS_THEN_REST) return PTX_ERR_INVALID_ARG;
    for (uint32_t c = 0; c < P; ++c)
        if (src_log[c] >= L) return PTX_ERR_INVALID_ARG;
    uint64_t* scr = (uint64_t*)calloc((size_t)P + 1, 8);
    uint32_t* ident = (uint32_t*)malloc(((size_t)P + 1) * 4);
    uint32_t* n_out = (uint32_t*)malloc(((size_t)P + 1) * 4);
    uint32_t* n_rows = (uint32_t*)malloc(((size_t)P + 1) * 4);
    if (!scr || !ident || !n_out || !n_rows) return -1;
    for (uint32_t c = 0; c < P; ++c) {
        scr[c + 1] = scr[c] + ptx_sync_scratch_words(b->chg_off[src_log[c] + 1] - b->chg_off[src_log[c]]);
        ident[c] = c;
    }
    const size_t lds_bytes = (size_t)ptx_version_lds_need(b->max_actors);
    uint32_t* scratch = (uint32_t*)malloc(scr[P] * 4 + 4);
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (lds_bytes + 63) & ~(size_t)63);
    if (!scratch || !lds) return -1;
    memset(scratch, 0xA5, scr[P] * 4);
    PtxVersionArgs V;
    memset(&V, 0, sizeof(V));
    PtxSyncArgs& A = V.S;
    A.log_off = b->log_off;
    A.chg_off = b->chg_off;
    A.chg_hdr = b->chg_hdr;
    A.chg_env = b->chg_env;
    A.chg_env_hi = b->chg_env_hi;
    A.max_actors = b->max_actors;
    A.n_pairs = P;
    A.src_log = src_log;
    A.dst_log = ident;
    A.scr_off = scr;
    A.scratch = scratch;
    A.status = status;
    A.n_admitted = n_out;
    A.n_rows = n_rows;
    A.lds_bytes = (uint32_t)lds_bytes;
    V.clocks = clocks;
    V.prefix = prefix;
    V.flags = flags;
    V.n_kept = n_kept;
    V.first_row = first_row;
    V.clocks_out = clocks_out;
    ptx_emu_reverse = reverse;
    for (uint32_t c = 0; c < P; ++c) {
        memset(lds, 0xA5, lds_bytes); /* LDS is not zero-initialised on the GPU either */
        ptx_version_plan_cut<0>(V, c, lds);
    }
    o_log_off[0] = o_chg_off[0] = 0;
    for (uint32_t c = 0; c < P; ++c) {
        o_chg_off[c + 1] = o_chg_off[c] + n_out[c];
        o_log_off[c + 1] = o_log_off[c] + n_rows[c];
    }
    PtxSyncGatherArgs G = {b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b, o_op_id, o_ref_a, o_ref_b, o_payload, o_action, o_mark_type,
                           o_side_a, o_side_b, o_chg_hdr, o_chg_env, b->chg_env_hi ? o_chg_env_hi : nullptr, o_log_off, o_chg_off};
    for (uint32_t c = 0; c < P; ++c) ptx_sync_gather_pair<0>(A, G, c);
    free(lds);
    free(scratch);
    free(n_rows);
    free(n_out);
    free(ident);
    free(scr);
    return 0;
}
