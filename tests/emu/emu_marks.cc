/*
 * Host emulation of the merge kernel WITH the admission marks of a resident batch (peritext_amd/csrc/merge_core.h ptx_adm_mark) — TEST TOOLING ONLY, like
 * emu_driver.cc, whose drivers clear the kernel arguments and so keep walking every change of every log.
 *
 * Built into tests/emu/libperitext_emu_marks.so by __graft_entry__.build() and loaded only by tests/test_emu_adm_marks.py.  The caller owns the marks — four
 * u32 per log, zero = nothing admitted yet — and plays the host library: it keeps them from one merge of a batch to the next and hands the records of a base
 * batch to the batch an append makes of it.  The kernel reads and writes them as 16-byte records, so they pass through an aligned copy here.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
extern "C" unsigned long long ptx_emu_marks_exact_walk_count() { return ptx_emu_exact_walks; }
#include "../../peritext_amd/csrc/merge_core.h"

/* every log of `b` through ptx_merge_log with causal admission; marks: [4 * n_logs] in / out, or NULL (no marks: every change is walked).  lean: the body of the
 * ptx_merge_kernel_lean* builds for the logs that qualify (the host's own rule, as in emu_driver.cc); rank / refs may be NULL then. */
extern "C" int ptx_emu_merge_marks(const ptx_batch* b, ptx_log_result* res, uint32_t* values, ptx_span* spans, ptx_cinterval* cints, uint32_t* rank, uint32_t* refs,
                                   uint32_t* marks, uint32_t lds_bytes, int reverse, int lean) {
    if (!b->chg_off || !b->chg_hdr || !b->chg_env || b->max_actors == 0) return 2;
    PtxMergeArgs A;
    memset(&A, 0, sizeof(A));
    A.log_off = b->log_off;
    A.op_id = b->op_id;
    A.ref_a = b->ref_a;
    A.ref_b = b->ref_b;
    A.payload = b->payload;
    A.action = b->action;
    A.mark_type = b->mark_type;
    A.side_a = b->side_a;
    A.side_b = b->side_b;
    A.chg_off = b->chg_off;
    A.chg_hdr = b->chg_hdr;
    A.chg_env = b->chg_env;
    A.chg_env_hi = b->chg_env_hi;
    A.max_actors = b->max_actors;
    A.res = res;
    A.out_values = values;
    A.out_spans = spans;
    A.out_cints = cints;
    A.out_rank = rank;
    A.out_refs = refs;
    A.n_logs = b->n_logs;
    A.lds_bytes = lds_bytes;
    const size_t L = b->n_logs ? b->n_logs : 1;
    ptx_log_hdr* hdr = (ptx_log_hdr*)calloc(L, sizeof(ptx_log_hdr)); /* what the library's census pre-pass does on the device */
    ptx_adm_mark* mk = marks ? (ptx_adm_mark*)aligned_alloc(64, (L * sizeof(ptx_adm_mark) + 63) & ~(size_t)63) : nullptr;
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (((size_t)lds_bytes + 63) & ~(size_t)63) + 64);
    if (!hdr || !lds || (marks && !mk)) return 1;
    for (uint32_t l = 0; l < b->n_logs; ++l) {
        const uint64_t b0 = b->log_off[l], b1 = b->log_off[l + 1];
        if (b->log_hdr) hdr[l] = b->log_hdr[l];
        else ptx_census_rows(b->op_id + b0, b->action + b0, b->mark_type + b0, b->payload + b0, b1 - b0, &hdr[l]);
    }
    A.log_hdr = hdr;
    if (marks) memcpy(mk, marks, (size_t)b->n_logs * sizeof(ptx_adm_mark));
    A.adm_marks = mk;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < b->n_logs; ++l) {
        memset(lds, 0xA5, lds_bytes); /* LDS is not zero-initialised on the GPU either */
        const uint64_t ks = ((uint64_t)hdr[l].max_counter + 1) * ((uint64_t)hdr[l].max_actor + 1);
        if (lean && !rank && !refs && ks <= 65536u && b->max_actors <= 3) ptx_merge_log<0, 0, false, true>(A, l, lds);
        else if (b->max_actors >= 8u && b->max_actors <= 15u) ptx_merge_log<2, 0>(A, l, lds);
        else ptx_merge_log<1, 0>(A, l, lds);
    }
    if (marks) memcpy(marks, mk, (size_t)b->n_logs * sizeof(ptx_adm_mark));
    free(mk);
    free(lds);
    free(hdr);
    return 0;
}
