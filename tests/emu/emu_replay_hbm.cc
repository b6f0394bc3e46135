/*
 * Host emulation of the HBM-state patch replay (peritext_amd/csrc/replay_hbm_core.h) — TEST TOOLING ONLY, like emu_driver.cc.
 *
 * Built into tests/emu/libperitext_emu_replay_hbm.so by __graft_entry__.build() and loaded only by tests/test_emu_replay_hbm.py.  The merge results it replays
 * come from libperitext_emu.so (helpers.emu_merge / emu_merge_big).  Every log of the batch goes through ptx_replay_log_hbm, whatever its size; the state
 * slices are filled with 0xA5 first: the kernel zeroes what it needs zeroed.
 */
#define PTX_EMU 1
#define PTX_PLATFORM_HEADER "../../tests/emu/ptx_platform_emu.h" /* resolved from peritext_amd/csrc/, where the #include stands */
#include <stdlib.h>
#include <string.h>
int ptx_emu_reverse = 0;
unsigned long long ptx_emu_exact_walks = 0;
#include "../../peritext_amd/csrc/merge_core.h"
#include "../../peritext_amd/csrc/replay_hbm_core.h"

/* patch_off = capacity offsets [n_logs + 1]; arena_cap > 0: `patches` holds arena_cap more records behind patch_off[n_logs] for the overflow extents and
 * ext_off[3 * n_logs] says where a log's extents are (as ptx_emu_replay_arena); refs_hi: the high halves of the boundary slots (NULL: a result without them);
 * first_row: NULL = whole streams */
extern "C" int ptx_emu_replay_hbm(const ptx_batch* b, const ptx_log_result* res, const uint32_t* rank, const uint32_t* refs, const uint32_t* refs_hi, const uint64_t* patch_off,
                                  ptx_patch* patches, ptx_patch_log* plogs, int reverse, const uint32_t* first_row, uint64_t arena_cap, uint64_t* ext_off) {
    PtxReplayHbmArgs HA;
    memset(&HA, 0, sizeof(HA));
    PtxReplayArgs& A = HA.R;
    unsigned long long arena_next = 0;
    A.first_row = first_row;
    A.arena_next = arena_cap ? &arena_next : nullptr;
    A.arena_base = b->n_logs ? patch_off[b->n_logs] : 0;
    A.arena_cap = arena_cap;
    A.ext_off = arena_cap ? ext_off : nullptr;
    A.log_off = b->log_off;
    A.op_id = b->op_id;
    A.ref_a = b->ref_a;
    A.ref_b = b->ref_b;
    A.payload = b->payload;
    A.action = b->action;
    A.mark_type = b->mark_type;
    A.side_a = b->side_a;
    A.side_b = b->side_b;
    A.res = res;
    A.elem_rank = rank;
    A.refs = refs;
    A.refs_hi = refs_hi;
    A.patch_off = patch_off;
    A.patches = patches;
    A.plogs = plogs;
    A.n_logs = b->n_logs;
    const uint32_t L = b->n_logs;
    ptx_log_hdr* hdr = (ptx_log_hdr*)calloc(L ? L : 1, sizeof(ptx_log_hdr));
    uint64_t* off = (uint64_t*)calloc((size_t)L + 1, 8);
    uint32_t* index = (uint32_t*)calloc(L ? L : 1, 4);
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t b0 = b->log_off[l], b1 = b->log_off[l + 1];
        if (b->log_hdr) hdr[l] = b->log_hdr[l];
        else ptx_census_rows(b->op_id + b0, b->action + b0, b->mark_type + b0, b->payload + b0, b1 - b0, &hdr[l]);
        off[l + 1] = off[l] + ptx_replay_hbm_units_hdr(hdr[l]);
        index[l] = l;
    }
    A.log_hdr = hdr;
    uint32_t* state = (uint32_t*)aligned_alloc(64, ((4 * off[L] + 63) & ~63ull) + 64);
    uint8_t* lds = (uint8_t*)aligned_alloc(64, PTX_REPLAY_HBM_LDS_BYTES + 64);
    if (!state || !lds) return 1;
    memset(state, 0xA5, 4 * off[L]);
    HA.state = state;
    HA.state_off = off;
    HA.log_index = index;
    HA.n_hbm = L;
    ptx_emu_reverse = reverse;
    for (uint32_t l = 0; l < L; ++l) {
        memset(lds, 0xA5, PTX_REPLAY_HBM_LDS_BYTES); /* LDS is not zero-initialised on the GPU either */
        ptx_replay_log_hbm<0>(HA, l, lds);
#if defined(__SANITIZE_ADDRESS__)
        ASAN_UNPOISON_MEMORY_REGION(lds, PTX_REPLAY_HBM_LDS_BYTES); /* (the bump allocator's padding marks of this log) */
#endif
    }
    free(lds);
    free(state);
    free(index);
    free(off);
    free(hdr);
    return 0;
}
/* u32 units of state scratch the host library sizes a log's slice with */
extern "C" uint64_t ptx_emu_replay_hbm_units(uint64_t n, uint64_t K, uint64_t Kc, uint64_t Kid) { return ptx_replay_hbm_units(n, K, Kc, Kid); }
extern "C" uint32_t ptx_emu_replay_hbm_lds_bytes() { return PTX_REPLAY_HBM_LDS_BYTES; }
