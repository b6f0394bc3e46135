/*
 * Host emulation of the merge kernel WITH the row index of a resident batch, the operand words of its mark ops AND the host's leave to take a standing log's
 * row-order checks as passed (peritext_amd/csrc/merge_core.h PtxMergeArgs::order_checks_once) — TEST TOOLING ONLY, like emu_markops.cc, whose driver leaves
 * that field 0 and so keeps running every check in every launch.
 *
 * Built into tests/emu/libperitext_emu_orderchecks.so by __graft_entry__.build() and loaded only by tests/test_emu_order_checks.py (emu_orderchecks_main.cc
 * drives the same entry under the sanitizers).  The caller owns the index and the operand words and plays the host library: the first merge of a batch gets
 * write = 1, the later ones write = 0 and, if it likes, once = 1.  The row-order checks of P3a / P3b are counted through PTX_NOTE_ORDER_CHECK, a hook of
 * merge_core.h that is empty everywhere else (once per delete of the pass behind P3a and of the rest loop, once per insert of P3b).
 *
 * PTX_ORDER_CHECKS_ONCE_FORM is 1 here: every body this driver runs may skip.  The product keeps the skip to the three-wave lean build, which never resolves
 * references; here the lean body skips and the general bodies, which are run with out_refs, show the other half of the condition — with references to resolve
 * nothing is skipped.  A general body that skips is not something the product ships.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
static unsigned long long g_order_checks = 0;
#define PTX_NOTE_ORDER_CHECK() (++g_order_checks)
#define PTX_ORDER_CHECKS_ONCE_FORM 1
#include "../../peritext_amd/csrc/merge_core.h"

extern "C" unsigned long long ptx_emu_orderchecks_words(unsigned long long n_ops, unsigned long long n_logs) { return ptx_row_index_words(n_ops, n_logs); }
extern "C" unsigned long long ptx_emu_orderchecks_bits_words(unsigned long long n_ops, unsigned long long n_logs) { return ptx_row_bits_words(n_ops, n_logs); }
extern "C" uint32_t ptx_emu_orderchecks_step_items(void) { return 2u; /* PTX_U of the bodies below (kThreads = 0) x the emulation's one thread */ }

/* every log of `b` through ptx_merge_log; index / bits / rows_indexed: the caller's index blocks, ops / stand: its operand words.  write: this merge is the
 * batch's one writer.  once: PtxMergeArgs::order_checks_once.  checks: optional [n_logs], the row-order checks each log made.  lean: the body of the
 * ptx_merge_kernel_lean* builds for the logs that qualify (the host's own rule, as in emu_driver.cc); otherwise the general body (no more than three actors) or
 * the many-actor ones. */
extern "C" int ptx_emu_merge_orderchecks(const ptx_batch* b, ptx_log_result* res, uint32_t* values, ptx_span* spans, ptx_cinterval* cints, uint32_t* rank, uint32_t* refs,
                                         uint32_t* index, uint32_t* bits, uint32_t* rows_indexed, uint64_t* ops, uint32_t* stand, int write, int once,
                                         unsigned long long* checks, uint32_t lds_bytes, int reverse, int lean) {
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
    const bool env = b->chg_off && b->chg_hdr && b->chg_env && b->max_actors;
    A.chg_off = env ? b->chg_off : nullptr;
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
    A.row_index = index;
    A.row_index_bits = bits;
    A.rows_indexed = rows_indexed;
    A.row_index_write = index && write ? 1u : 0u;
    A.mark_ops = index ? ops : nullptr;
    A.mark_ops_stand = index && ops ? stand : nullptr;
    A.order_checks_once = once ? 1u : 0u;
    const size_t L = b->n_logs ? b->n_logs : 1;
    ptx_log_hdr* hdr = (ptx_log_hdr*)calloc(L, sizeof(ptx_log_hdr)); /* what the library's census pre-pass does on the device */
    uint8_t* lds = (uint8_t*)aligned_alloc(64, (((size_t)lds_bytes + 63) & ~(size_t)63) + 64);
    if (!hdr || !lds) return 1;
    for (uint32_t l = 0; l < b->n_logs; ++l) {
        const uint64_t b0 = b->log_off[l], b1 = b->log_off[l + 1];
        if (b->log_hdr) hdr[l] = b->log_hdr[l];
        else ptx_census_rows(b->op_id + b0, b->action + b0, b->mark_type + b0, b->payload + b0, b1 - b0, &hdr[l]);
    }
    A.log_hdr = hdr;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < b->n_logs; ++l) {
#if defined(__SANITIZE_ADDRESS__)
        ASAN_UNPOISON_MEMORY_REGION(lds, lds_bytes); /* (the padding marks the bump allocator left for the log before) */
#endif
        memset(lds, 0xA5, lds_bytes); /* LDS is not zero-initialised on the GPU either */
        const unsigned long long g0 = g_order_checks;
        const uint64_t ks = ((uint64_t)hdr[l].max_counter + 1) * ((uint64_t)hdr[l].max_actor + 1);
        if (lean && !rank && !refs && ks <= 65536u && (!env || b->max_actors <= 3)) ptx_merge_log<0, 0, false, true>(A, l, lds);
        else if (env && b->max_actors >= 8u && b->max_actors <= 15u) ptx_merge_log<2, 0>(A, l, lds);
        else if (env && b->max_actors > 3u) ptx_merge_log<1, 0>(A, l, lds);
        else ptx_merge_log<0, 0>(A, l, lds);
        if (checks) checks[l] = g_order_checks - g0;
    }
    free(lds);
    free(hdr);
    return 0;
}
