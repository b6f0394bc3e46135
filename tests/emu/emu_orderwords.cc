/*
 * Host emulation of the merge kernel WITH the row index of a resident batch, the operand words of its mark ops AND its order words (peritext_amd/csrc/merge_core.h
 * ptx_order_word: per element its row and its document position, and the tombstone bitmap, kept by the batch's first merge so that later merges run nothing of
 * P3, the causal tree) — TEST TOOLING ONLY, like emu_orderchecks.cc, whose driver passes no order words and so keeps running P3 in every launch.
 *
 * Built into tests/emu/libperitext_emu_orderwords.so by __graft_entry__.build() and loaded only by tests/test_emu_order_words.py (emu_orderwords_main.cc drives
 * the same entry under the sanitizers).  The caller owns every block and plays the host library: the first merge of a batch gets write = 1, the later ones
 * write = 0.  Three hooks of merge_core.h that are empty everywhere else are counted per log: PTX_NOTE_TREE_PASS (the log enters P3), PTX_NOTE_MARK_GATHER (P5a
 * gathers one mark op's operands through its row) and PTX_NOTE_ORDER_CHECK (one row-order check of P3a / P3b).
 *
 * PTX_ORDER_WORDS_FORM and PTX_ORDER_CHECKS_ONCE_FORM are 1 here: every body this driver runs may read the words.  The product keeps both to the three-wave lean
 * build, which never resolves references; here the lean body reads and the general bodies, which are run with out_refs, show the other half of the condition —
 * with references to resolve P3 runs.  A general body that reads the words is not something the product ships.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
static unsigned long long g_tree_passes = 0, g_mark_gathers = 0, g_order_checks = 0;
#define PTX_NOTE_TREE_PASS() (++g_tree_passes)
#define PTX_NOTE_MARK_GATHER() (++g_mark_gathers)
#define PTX_NOTE_ORDER_CHECK() (++g_order_checks)
#define PTX_ORDER_CHECKS_ONCE_FORM 1
#define PTX_ORDER_WORDS_FORM 1
#include "../../peritext_amd/csrc/merge_core.h"

extern "C" unsigned long long ptx_emu_orderwords_words(unsigned long long n_ops, unsigned long long n_logs) { return ptx_row_index_words(n_ops, n_logs); }
extern "C" unsigned long long ptx_emu_orderwords_bits_words(unsigned long long n_ops, unsigned long long n_logs) { return ptx_row_bits_words(n_ops, n_logs); }
extern "C" unsigned long long ptx_emu_orderwords_off(unsigned long long row_off, unsigned long long log) { return ptx_row_index_off(row_off, log); }
extern "C" unsigned long long ptx_emu_orderwords_bits_off(unsigned long long row_off, unsigned long long log) { return ptx_row_bits_off(row_off, log); }
extern "C" uint32_t ptx_emu_orderwords_load_step(void) { return 8u; /* elements of one step of the reader's load loop: the emulation's one thread x 2 loads x 4 words */ }

/* every log of `b` through ptx_merge_log; index / bits / rows_indexed: the caller's index blocks, ops / stand: its operand words, ow / ob / ostand: its order
 * words, tombstone words and their word per log (all three or none).  write: this merge is the batch's one writer.  once: PtxMergeArgs::order_checks_once.
 * counts: optional [3 * n_logs], per log the tree passes, the mark gathers and the row-order checks it made.  lean: the body of the ptx_merge_kernel_lean* builds
 * for the logs that qualify (the host's own rule, as in emu_driver.cc); otherwise the general body (no more than three actors) or the many-actor ones. */
extern "C" int ptx_emu_merge_orderwords(const ptx_batch* b, ptx_log_result* res, uint32_t* values, ptx_span* spans, ptx_cinterval* cints, uint32_t* rank, uint32_t* refs,
                                        uint32_t* index, uint32_t* bits, uint32_t* rows_indexed, uint64_t* ops, uint32_t* stand, uint32_t* ow, uint32_t* ob,
                                        uint32_t* ostand, int write, int once, unsigned long long* counts, uint32_t lds_bytes, int reverse, int lean) {
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
    const bool ord = index && ops && ow && ob && ostand;
    A.order_words = ord ? ow : nullptr;
    A.order_bits = ord ? ob : nullptr;
    A.order_stands = ord ? ostand : nullptr;
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
        const unsigned long long t0 = g_tree_passes, m0 = g_mark_gathers, c0 = g_order_checks;
        const uint64_t ks = ((uint64_t)hdr[l].max_counter + 1) * ((uint64_t)hdr[l].max_actor + 1);
        if (lean && !rank && !refs && ks <= 65536u && (!env || b->max_actors <= 3)) ptx_merge_log<0, 0, false, true>(A, l, lds);
        else if (env && b->max_actors >= 8u && b->max_actors <= 15u) ptx_merge_log<2, 0>(A, l, lds);
        else if (env && b->max_actors > 3u) ptx_merge_log<1, 0>(A, l, lds);
        else ptx_merge_log<0, 0>(A, l, lds);
        if (counts) {
            counts[3u * l] = g_tree_passes - t0;
            counts[3u * l + 1u] = g_mark_gathers - m0;
            counts[3u * l + 2u] = g_order_checks - c0;
        }
    }
    free(lds);
    free(hdr);
    return 0;
}
