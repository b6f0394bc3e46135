/*
 * peritext_hip.hip — gfx950 kernels + the C ABI of include/peritext_hip.h (libperitext_hip.so).
 *
 * Kernel: ptx_merge_kernel — ONE workgroup per replica-log; the whole log lives in LDS while the
 * causal tree, tombstone scan, mark sweep and span RLE run (merge_core.h).  HBM traffic is the
 * compulsory one: 32 B/op read once, outputs written once.  No MFMA: this is integer/indexing work
 * bounded by LDS latency and HBM bandwidth.
 *
 * Host side: a context owns one HIP stream and its allocations; batches and results are explicit
 * device-resident objects so that a benchmark can keep the op log in HBM and time only the merge.
 * There is no CPU path in this library: without a gfx950 device ptx_create fails.
 */
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <atomic>
#include <mutex>
#include <set>
#include <unordered_map>
#include <string>
#include <vector>

#include "merge_core.h"
#include "biglog_core.h"
#include "replay_core.h"
#include "replay_hbm_core.h"
#include "gen_core.h"
#include "change_core.h"
#include "change_prep_core.h"
#include "cursor_core.h"
#include "rootmap_core.h"
#include "sync_core.h"
#include "version_core.h"
#include "accum_core.h"
#include "text_core.h"
#include "find_core.h"
#include "slice_core.h"
#include "view_core.h"
#include "replace_core.h"
#include "markrun_core.h"

/* ------------------------------------------------------------------------------------------------ */
/* kernels                                                                                          */
/* ------------------------------------------------------------------------------------------------ */

/* One body, several register budgets: __launch_bounds__(T, W) = at most T threads per workgroup and at
 * least W waves per SIMD resident, i.e. the compiler must stay within 512/W VGPRs (MI355X_MICROARCH.md
 * "Register files"). */
#ifndef PTX_W
#define PTX_W 1 /* minimum waves per SIMD the register allocation of ptx_merge_kernel must allow (8: ten 3-wave logs per CU need it; costs SGPR spills) */
#endif
/* Scalar registers decide the wave slots too, and not as the compiler's occupancy figure says: measured on MI355X (tools/micro/reg_occupancy.hip,
 * profiles/r03_p_*) a kernel of up to 96 SGPRs (vcc etc. included) holds 7 waves per SIMD, one of 98 or more holds 6 — 24 waves per CU, i.e. exactly the
 * eight 3-wave logs that the LDS window of a 4 096-op log allows anyway.  Where the LDS would allow more waves than 24 (short logs), the host launches
 * the "_w7" builds: the same body held to 90 SGPRs (+ vcc ...; costs ~70 more SGPR spills into VGPR lanes, 1-2 % at equal occupancy). */
#ifndef PTX_W7_SGPRS
#define PTX_W7_SGPRS 96 /* (granted: 94 with vcc etc. — the last count that still holds 7 waves per SIMD; 90 cost 50 more spills) */
#endif
#define PTX_SGPRS_W7 __attribute__((amdgpu_num_sgpr(PTX_W7_SGPRS)))
#define PTX_MERGE_KERNEL(name, T, W, MANY, KT, DIAG) PTX_MERGE_KERNEL_A(name, T, W, MANY, KT, DIAG, )
#define PTX_MERGE_KERNEL_A(name, T, W, MANY, KT, DIAG, PTX_SGPR_CAP) PTX_MERGE_KERNEL_L(name, T, W, MANY, KT, DIAG, false, PTX_SGPR_CAP)
#define PTX_MERGE_KERNEL_L(name, T, W, MANY, KT, DIAG, LEAN, PTX_SGPR_CAP)                                     \
    extern "C" __global__ void __launch_bounds__(T, W) PTX_SGPR_CAP name(PtxMergeArgs A) { \
        extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];              \
        /* one workgroup per log (grid == n_logs): no grid-stride loop, so that nothing is hoisted \
           out of it and kept in registers for the whole kernel */                    \
        if (blockIdx.x < A.n_logs) ptx_merge_log<MANY, KT, DIAG, LEAN>(A, A.log_index ? A.log_index[blockIdx.x] : blockIdx.x, ptx_lds); \
    }
PTX_MERGE_KERNEL(ptx_merge_kernel, 1024, PTX_W, 0, 0, false)     /* any launch shape (blockDim.x read at run time) */
PTX_MERGE_KERNEL(ptx_merge_kernel_rest, 1024, 1, 0, 0, false) /* the same kernel under another name: the second launch of a split batch (the few logs
                                                                    with a larger LDS window), so that per-kernel statistics of a trace keep the two apart */
PTX_MERGE_KERNEL_A(ptx_merge_kernel_w7, 1024, PTX_W, 0, 0, false, PTX_SGPRS_W7)      /* the same two at 7 waves per SIMD (see above) */
PTX_MERGE_KERNEL_A(ptx_merge_kernel_rest_w7, 1024, 1, 0, 0, false, PTX_SGPRS_W7)
/* Round 5: the LEAN builds, one per usual launch shape (threads per log known at compile time: the loop strides fold; a one-wave log has no s_barrier at all).
 * For batches whose every log has 16-bit id keys (census) merged without elem_rank / resolved references (PTX_FLAG_NO_ELEM_RANK): neither the wide-key paths nor
 * the two optional outputs are in the code — 84 instead of 113 scalar registers spilled at the 96 that 7 waves per SIMD allow.  Measured same box against the
 * general build (profiles/r05_b_*): config #4 -1.2 %, #3 (two waves per log) -4.2 %, #2 (one wave) -4.9 %. */
/* Round 6: the one-wave build at EIGHT waves per SIMD (64 VGPRs, 80 SGPRs: 78 granted).  A one-wave log is a chain of fixed latencies on a SIMD it
 * shares with the other resident logs, and its LDS window (4 KB for a 256-op log, 10 KB for a 1K-op one) allows 32 waves per CU: 32 instead of 28 one-wave logs,
 * 16 instead of 14 two-wave ones.  Same box: config #2 -4.9 % (the ~70 scalar registers it spills cost less than the four more logs bring; the
 * three-wave build stays at seven: nine logs per CU are 27 waves). */
#ifndef PTX_LEAN64_W
#define PTX_LEAN64_W 8
#endif
#ifndef PTX_LEAN64_SGPRS
#define PTX_LEAN64_SGPRS 80
#endif
PTX_MERGE_KERNEL_L(ptx_merge_kernel_lean64, 64, PTX_LEAN64_W, 0, 64, false, true, __attribute__((amdgpu_num_sgpr(PTX_LEAN64_SGPRS))))
/* The two-wave build likewise since the last session of round 6 (64 VGPRs, 78 SGPRs granted, nothing in scratch — its admission walk fits now): 16 instead of 14 logs
 * per CU where the LDS window allows; same box config #3 -4.6 % (2.912 -> 2.779 ms, same results). */
#ifndef PTX_LEAN128_W
#define PTX_LEAN128_W 8
#endif
#ifndef PTX_LEAN128_SGPRS
#define PTX_LEAN128_SGPRS 80
#endif
PTX_MERGE_KERNEL_L(ptx_merge_kernel_lean128, 128, PTX_LEAN128_W, 0, 128, false, true, __attribute__((amdgpu_num_sgpr(PTX_LEAN128_SGPRS))))
#ifndef PTX_LEAN192_W
#define PTX_LEAN192_W PTX_W
#endif
#ifndef PTX_LEAN192_SGPRS
#define PTX_LEAN192_SGPRS PTX_W7_SGPRS
#endif
PTX_MERGE_KERNEL_L(ptx_merge_kernel_lean192, 192, PTX_LEAN192_W, 0, 192, false, true, __attribute__((amdgpu_num_sgpr(PTX_LEAN192_SGPRS))))
/* round 6 (last session): the four-wave lean build — 8K-op logs (BASELINE config #5: four 39 KB logs per CU) and 4K-op logs that keep their text (`rich4k`); their LDS
 * window, not the registers, bounds the resident logs, so the build takes what registers it wants */
PTX_MERGE_KERNEL_L(ptx_merge_kernel_lean256, 256, 1, 0, 256, false, true, )
PTX_MERGE_KERNEL(ptx_merge_kernel_many, 1024, 1, 1, 0, false) /* + causal admission for documents with more than three actors: a one-pass walk up to seven, the (actor, seq) table beyond fifteen */
PTX_MERGE_KERNEL(ptx_merge_kernel_many_wide, 1024, 1, 2, 0, false) /* the same for documents of eight to fifteen actors (walks over 24- and 32-byte envelope rows) */
#ifdef PTX_DIAG /* (diagnostic builds only) the stamps of the LEAN builds: the same bodies as ptx_merge_kernel_lean64 / 128 / 192 with the phase stamps on */
PTX_MERGE_KERNEL_L(ptx_merge_kernel_diag64, 64, PTX_W, 0, 64, true, true, PTX_SGPRS_W7)
PTX_MERGE_KERNEL_L(ptx_merge_kernel_diag128, 128, PTX_W, 0, 128, true, true, PTX_SGPRS_W7)
PTX_MERGE_KERNEL_L(ptx_merge_kernel_diag192, 192, PTX_W, 0, 192, true, true, PTX_SGPRS_W7)
#endif
PTX_MERGE_KERNEL(ptx_merge_kernel_diag, 1024, PTX_W, 0, 0, true)  /* (the admission of the product kernel — with the table path of the many-actor build it needs 105 VGPRs and its phase stamps would be taken at 4 waves per SIMD —) + phase cycle stamps / early exit (ptx_merge_phase_cycles, PTX_STOP_AFTER) */
/* (ptx_merge_log<MANY, T> can fold the workgroup size T in at compile time; measured on MI355X the specialised builds
 * issue ~1 % fewer instructions but need twice the VGPRs unless PTX_U=1, so only the run-time-sized builds are shipped) */

/* Logs beyond one CU's LDS (biglog_core.h): one workgroup of PTX_BIG_THREADS per log, the working set in a slice of HBM scratch */
#define PTX_BIG_THREADS 1024
extern "C" __global__ void __launch_bounds__(PTX_BIG_THREADS) ptx_merge_big_kernel(PtxMergeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_logs) ptx_big_merge_log<false>(A, A.log_index[blockIdx.x], A.big_scratch + A.big_off[blockIdx.x], A.big_off[blockIdx.x + 1] - A.big_off[blockIdx.x], ptx_lds);
}
/* Round 5 (VERDICT r4 missing #3): ONE large log merged by ALL the workgroups of a cooperative launch — the same body, its loops striding over the grid's threads,
 * its barriers grid barriers (ptx_grid_sync), its header in the scratch slice.  The host launches one such kernel per log of at least PTX_BIG_GRID_ROWS rows
 * (hipLaunchCooperativeKernel: every workgroup is resident, so the spinning barrier cannot starve one); the workgroup count grows with the log. */
#define PTX_BIG_GRID_THREADS 256
#define PTX_BIG_GRID_MAX_WGS 64u
#define PTX_BIG_GRID_ROWS 16384u
#define PTX_BIG_TEAM_MAX (PTX_BIG_GRID_THREADS * PTX_BIG_GRID_MAX_WGS) /* >= PTX_BIG_THREADS: the largest team a log's scratch is sized for */
extern "C" __global__ void __launch_bounds__(PTX_BIG_GRID_THREADS) ptx_merge_big_grid_kernel(PtxMergeArgs A) {
    ptx_big_merge_log<true>(A, A.log_index[0], A.big_scratch + A.big_off[0], A.big_off[1] - A.big_off[0], nullptr);
}

/* Patch-stream replay (replay_core.h): one 64-thread workgroup (one wave) per log, sequential in application order */
#ifndef PTX_REPLAY_GWIN_ABOVE
#define PTX_REPLAY_GWIN_ABOVE 5632u /* LDS bytes per log beyond which the replay's per-slot link urls, its tables of applied mark ops and the comment ops' id tables move to global memory (below it the wave slots of a CU — 24 at this kernel's 106 SGPRs, see PTX_SGPRS_W7 —, not its LDS, bound the resident logs) */
#endif
#ifndef PTX_REPLAY_THREADS
#define PTX_REPLAY_THREADS 64
#endif
/* (round 3's kernel held to 90 SGPRs for 28 instead of 24 wave slots per CU — see PTX_SGPRS_W7 — was SLOWER, its spills sit on the sequential chain; round 4's
 * 6.2 KB of LDS per 4K-op log allow 24 logs per CU, exactly what its 106 SGPRs do) */
static_assert(PTX_REPLAY_THREADS == 64, "replay_core.h is written for ONE wave per log: wave-wide searches, register counters, a one-wave scan without LDS scratch");
extern "C" __global__ void __launch_bounds__(PTX_REPLAY_THREADS) ptx_replay_kernel(PtxReplayArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_logs) ptx_replay_log<PTX_REPLAY_THREADS, false>(A, blockIdx.x, ptx_lds);
}
/* the same with the per-slot link urls, the op tables and the comment ops' id tables in global memory (A.win_scratch): 20 of a 4K-op log's 26 KB of LDS, i.e. 24 logs per CU instead of six */
extern "C" __global__ void __launch_bounds__(PTX_REPLAY_THREADS) ptx_replay_kernel_gwin(PtxReplayArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_logs) ptx_replay_log<PTX_REPLAY_THREADS, true>(A, blockIdx.x, ptx_lds);
}
/* round 6: the wide build — ranks and boundary slots 32 bits wide — for batches with a log of more than 32 766 list elements or 65 534 rows (merged by the HBM-staged
 * kernel, which hands the slots' high halves over in ptx_dresult.refs_hi); urls and op tables always in global memory */
extern "C" __global__ void __launch_bounds__(PTX_REPLAY_THREADS) ptx_replay_kernel_wide(PtxReplayArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_logs) ptx_replay_log<PTX_REPLAY_THREADS, true, true>(A, blockIdx.x, ptx_lds);
}

/* the logs whose replay state does not fit the LDS (replay_hbm_core.h): the state in a slice of A.state per log, a fixed 12 KB of static LDS; one wave per log of
 * A.log_index */
extern "C" __global__ void __launch_bounds__(PTX_REPLAY_THREADS) ptx_replay_kernel_hbm(PtxReplayHbmArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_hbm_lds[PTX_REPLAY_HBM_LDS_BYTES];
    if (blockIdx.x < A.n_hbm) ptx_replay_log_hbm<PTX_REPLAY_THREADS>(A, blockIdx.x, ptx_hbm_lds);
}

/* the records of every log — first its own capacity [cap_off[l], cap_off[l + 1]), then its overflow extent from ext_off[l] — packed to out_off[l]; the logs from
 * first_log on, into a buffer that starts at record out_base of the packed stream (the whole stream in one go unless device memory is short) */
extern "C" __global__ void __launch_bounds__(256) ptx_patch_pack_kernel(const ptx_patch* src, const uint64_t* cap_off, const uint64_t* ext_off, const uint64_t* out_off, ptx_patch* dst,
                                                                        uint32_t first_log, uint64_t out_base) {
    const uint32_t l = first_log + blockIdx.x;
    const uint64_t c0 = cap_off[l], cap = cap_off[l + 1] - c0, o0 = out_off[l] - out_base, n = out_off[l + 1] - out_off[l];
    const uint64_t x0 = ext_off[3 * (uint64_t)l], x1 = ext_off[3 * (uint64_t)l + 1], xcap = ext_off[3 * (uint64_t)l + 2];
    for (uint64_t i = threadIdx.x; i < n; i += 256) dst[o0 + i] = i < cap ? src[c0 + i] : i - cap < xcap ? src[x0 + (i - cap)] : src[x1 + (i - cap - xcap)];
}

/* On-device change() / PTXGEN (gen_core.h): one 64-thread workgroup (one wave) per document */
#ifndef PTX_GEN_SGPR_CAP
#define PTX_GEN_SGPR_CAP
#endif
extern "C" __global__ void __launch_bounds__(64) PTX_GEN_SGPR_CAP ptx_gen_kernel(PtxGenArgs A) { /* documents of up to four replicas */
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_docs) ptx_gen_doc<64, 4>(A, blockIdx.x, ptx_lds);
}
extern "C" __global__ void __launch_bounds__(64) ptx_gen_kernel_r8(PtxGenArgs A) { /* five to eight replicas: the per-replica state twice as wide */
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_docs) ptx_gen_doc<64, PTX_GEN_MAX_R>(A, blockIdx.x, ptx_lds);
}
/* change() for caller-supplied InputOperations (change_core.h): one 64-thread workgroup (one wave) per replica log */
extern "C" __global__ void __launch_bounds__(64) ptx_change_kernel(PtxChangeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_logs) ptx_change_log<64>(A, blockIdx.x, ptx_lds);
}
/* ... and its preparation for InputOperations that are resident (change_prep_core.h): a lane per entry of the two offset arrays checks them, one wave per log
 * counts the rows its Changes will make, checks its inserts against `values` and folds its LDS need into the launch's */
extern "C" __global__ void __launch_bounds__(256) ptx_change_offsets_check_kernel(PtxChangePrepArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < ptx_change_offsets_entries(A)) ptx_change_offsets_check_one(A, i);
}
extern "C" __global__ void __launch_bounds__(64) ptx_change_prep_kernel(PtxChangePrepArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_prep_lds[PTX_CHANGE_PREP_LDS_BYTES];
    if (blockIdx.x < A.n_logs) ptx_change_prep_log<64>(A, blockIdx.x, ptx_prep_lds);
}

/* the sync between two replicas (sync_core.h): one wave per pair plans (missing changes in retry order), one workgroup per pair gathers their rows */
#define PTX_SYNC_GATHER_THREADS 256
extern "C" __global__ void __launch_bounds__(64) ptx_sync_plan_kernel(PtxSyncArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_pairs) ptx_sync_plan_pair<64>(A, blockIdx.x, ptx_lds);
}
extern "C" __global__ void __launch_bounds__(PTX_SYNC_GATHER_THREADS) ptx_sync_gather_kernel(PtxSyncArgs A, PtxSyncGatherArgs G) {
    if (blockIdx.x < A.n_pairs) ptx_sync_gather_pair<PTX_SYNC_GATHER_THREADS>(A, G, blockIdx.x);
}
/* a resident log at a past version (version_core.h): one wave per cut plans (the kept changes, the rest behind them); ptx_sync_gather_kernel copies */
extern "C" __global__ void __launch_bounds__(64) ptx_version_plan_kernel(PtxVersionArgs V) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < V.S.n_pairs) ptx_version_plan_cut<64>(V, blockIdx.x, ptx_lds);
}

/* patch streams back into canonical rows (accum_core.h): one wave per log, the state in the log's LDS window or — a log beyond one CU's LDS, or
 * PTX_FLAG_ACCUM_HBM_STATE — in a slice of global scratch; the same walk */
extern "C" __global__ void __launch_bounds__(64) ptx_accum_kernel(PtxAccumArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_launch) ptx_accum_log<64>(A, blockIdx.x, ptx_lds);
}
extern "C" __global__ void __launch_bounds__(64) ptx_accum_kernel_hbm(PtxAccumArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_accum_lds[PTX_ACCUM_HBM_LDS_BYTES];
    if (blockIdx.x < A.n_launch) ptx_accum_log_hbm<64>(A, blockIdx.x, ptx_accum_lds);
}

/* the map objects of a replica (rootmap_core.h): one wave per replica log; a first kernel counts the map rows (capacity of the entry rows) */
extern "C" __global__ void __launch_bounds__(64) ptx_rootmap_kernel(PtxRootArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_logs) ptx_rootmap_log<64>(A, blockIdx.x, ptx_lds);
}
__global__ void ptx_rootmap_count_kernel(const uint64_t* log_off, const uint8_t* action, uint32_t n_logs, uint32_t* counts) {
    const uint32_t log = blockIdx.x;
    if (log >= n_logs) return;
    const uint64_t b0 = log_off[log], b1 = log_off[log + 1];
    uint32_t c = 0;
    for (uint64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x) {
        const uint32_t a = action[i];
        c += (a == PTX_ACT_MAPSET || a == PTX_ACT_MAPDEL || a == PTX_ACT_MAKELIST) ? 1u : 0u;
    }
    c = ptx_wave_total(c); /* one wave per log */
    if (threadIdx.x == 0) counts[log] = c;
}

/* cursor resolution (cursor_core.h): one workgroup per replica log that has queries */
#define PTX_CURSOR_THREADS 128
extern "C" __global__ void __launch_bounds__(PTX_CURSOR_THREADS) ptx_cursor_kernel(PtxCursorArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ptx_lds[];
    if (blockIdx.x < A.n_groups) ptx_cursor_group<PTX_CURSOR_THREADS>(A, blockIdx.x, ptx_lds);
}

/* envelope of a generated batch: capacity layout (rows_per_log entries per log) -> compact */
__global__ void ptx_gen_compact_kernel(const uint64_t* chg_off, uint32_t rows_per_log, uint32_t R, const uint32_t* sh, const uint16_t* se, uint32_t* dh, uint16_t* de) {
    const uint32_t log = blockIdx.x, es = PTX_ENV_STRIDE(R);
    const uint64_t c0 = chg_off[log], c1 = chg_off[log + 1], s0 = (uint64_t)log * rows_per_log;
    for (uint64_t i = threadIdx.x; i < c1 - c0; i += blockDim.x) dh[c0 + i] = sh[s0 + i];
    for (uint64_t i = threadIdx.x; i < (c1 - c0) * es; i += blockDim.x) de[c0 * es + i] = se[s0 * es + i];
}
__global__ void ptx_regular_offsets_kernel(uint64_t* dst, uint32_t n, uint64_t stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) dst[i] = (uint64_t)i * stride;
}

/* streaming append: new log l = old log l followed by the appended rows of log l */
__global__ void ptx_append_offsets_kernel(const uint64_t* a, const uint64_t* b, uint64_t* dst, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) dst[i] = a[i] + b[i];
}
template <class T>
__device__ void ptx_append_col(const T* a, uint64_t a0, uint64_t na, const T* b, uint64_t b0, uint64_t nb, T* dst, uint64_t d0, uint64_t width) {
    for (uint64_t i = threadIdx.x; i < na * width; i += blockDim.x) dst[d0 * width + i] = a[a0 * width + i];
    for (uint64_t i = threadIdx.x; i < nb * width; i += blockDim.x) dst[(d0 + na) * width + i] = b[b0 * width + i];
}
struct PtxAppendCols {
    const uint64_t *op_id, *ref_a, *ref_b;
    const uint32_t* payload;
    const uint8_t *action, *mark_type, *side_a, *side_b;
    const uint32_t* chg_hdr;
    const uint16_t* chg_env;
    const uint16_t* chg_env_hi; /* may be NULL: zeros */
};
struct PtxAppendDst {
    uint64_t *op_id, *ref_a, *ref_b;
    uint32_t* payload;
    uint8_t *action, *mark_type, *side_a, *side_b;
    uint32_t* chg_hdr;
    uint16_t* chg_env;
    uint16_t* chg_env_hi; /* NULL: the destination has no wide column */
};
/* the wide envelope column of an appended batch: a side that has none contributes zeros */
__device__ void ptx_append_hi(const uint16_t* a, uint64_t a0, uint64_t na, const uint16_t* b, uint64_t b0, uint64_t nb, uint16_t* dst, uint64_t d0, uint64_t width) {
    for (uint64_t i = threadIdx.x; i < na * width; i += blockDim.x) dst[d0 * width + i] = a ? a[a0 * width + i] : (uint16_t)0;
    for (uint64_t i = threadIdx.x; i < nb * width; i += blockDim.x) dst[(d0 + na) * width + i] = b ? b[b0 * width + i] : (uint16_t)0;
}
__global__ void ptx_append_rows_kernel(PtxAppendCols A, const uint64_t* a_off, const uint64_t* a_coff, PtxAppendCols B, const uint64_t* b_off, const uint64_t* b_coff,
                                       PtxAppendDst D, const uint64_t* d_off, const uint64_t* d_coff, uint32_t max_actors) {
    const uint32_t l = blockIdx.x;
    const uint64_t a0 = a_off[l], na = a_off[l + 1] - a0, b0 = b_off[l], nb = b_off[l + 1] - b0, d0 = d_off[l];
    ptx_append_col(A.op_id, a0, na, B.op_id, b0, nb, D.op_id, d0, 1);
    ptx_append_col(A.ref_a, a0, na, B.ref_a, b0, nb, D.ref_a, d0, 1);
    ptx_append_col(A.ref_b, a0, na, B.ref_b, b0, nb, D.ref_b, d0, 1);
    ptx_append_col(A.payload, a0, na, B.payload, b0, nb, D.payload, d0, 1);
    ptx_append_col(A.action, a0, na, B.action, b0, nb, D.action, d0, 1);
    ptx_append_col(A.mark_type, a0, na, B.mark_type, b0, nb, D.mark_type, d0, 1);
    ptx_append_col(A.side_a, a0, na, B.side_a, b0, nb, D.side_a, d0, 1);
    ptx_append_col(A.side_b, a0, na, B.side_b, b0, nb, D.side_b, d0, 1);
    if (a_coff) {
        const uint64_t ac0 = a_coff[l], nac = a_coff[l + 1] - ac0, bc0 = b_coff[l], nbc = b_coff[l + 1] - bc0, dc0 = d_coff[l];
        ptx_append_col(A.chg_hdr, ac0, nac, B.chg_hdr, bc0, nbc, D.chg_hdr, dc0, 1);
        ptx_append_col(A.chg_env, ac0, nac, B.chg_env, bc0, nbc, D.chg_env, dc0, (uint64_t)PTX_ENV_STRIDE(max_actors));
        if (D.chg_env_hi) ptx_append_hi(A.chg_env_hi, ac0, nac, B.chg_env_hi, bc0, nbc, D.chg_env_hi, dc0, (uint64_t)PTX_ENV_STRIDE(max_actors));
    }
}

/* the first rows[l] rows (chgs[l] envelope rows) of every log of a capacity-layout batch -> a compact batch */
__global__ void ptx_take_rows_kernel(PtxAppendCols S, const uint64_t* s_off, const uint64_t* s_coff, const uint32_t* rows, const uint32_t* chgs, PtxAppendDst D,
                                     const uint64_t* d_off, const uint64_t* d_coff, uint32_t max_actors) {
    const uint32_t l = blockIdx.x;
    const uint64_t s0 = s_off[l], d0 = d_off[l], nr = rows[l];
    ptx_append_col(S.op_id, s0, nr, S.op_id, 0, 0, D.op_id, d0, 1);
    ptx_append_col(S.ref_a, s0, nr, S.ref_a, 0, 0, D.ref_a, d0, 1);
    ptx_append_col(S.ref_b, s0, nr, S.ref_b, 0, 0, D.ref_b, d0, 1);
    ptx_append_col(S.payload, s0, nr, S.payload, 0, 0, D.payload, d0, 1);
    ptx_append_col(S.action, s0, nr, S.action, 0, 0, D.action, d0, 1);
    ptx_append_col(S.mark_type, s0, nr, S.mark_type, 0, 0, D.mark_type, d0, 1);
    ptx_append_col(S.side_a, s0, nr, S.side_a, 0, 0, D.side_a, d0, 1);
    ptx_append_col(S.side_b, s0, nr, S.side_b, 0, 0, D.side_b, d0, 1);
    const uint64_t sc0 = s_coff[l], dc0 = d_coff[l], nc = chgs[l];
    ptx_append_col(S.chg_hdr, sc0, nc, S.chg_hdr, 0, 0, D.chg_hdr, dc0, 1);
    ptx_append_col(S.chg_env, sc0, nc, S.chg_env, 0, 0, D.chg_env, dc0, (uint64_t)PTX_ENV_STRIDE(max_actors));
    if (D.chg_env_hi) ptx_append_hi(S.chg_env_hi, sc0, nc, nullptr, 0, 0, D.chg_env_hi, dc0, (uint64_t)PTX_ENV_STRIDE(max_actors));
}

/* Census pre-pass: one workgroup per log.  compute != 0: derive the log header from the rows (batches
 * that came without one); always: fold the log's LDS requirement and row count into shape[0..1]. */
__global__ void __launch_bounds__(256) ptx_census_kernel(const uint64_t* log_off, const uint64_t* op_id, const uint8_t* action, const uint8_t* mark_type,
                                                          const uint32_t* payload, ptx_log_hdr* hdr, uint32_t* shape, int compute, const uint64_t* chg_off, uint32_t max_actors,
                                                          uint32_t* need_per_log, uint64_t n_ops, uint64_t* big_need_per_log, uint32_t max_lds, const uint16_t* chg_env_hi) {
    __shared__ uint32_t sh[9];
    __shared__ uint32_t wide;
    const uint32_t log = blockIdx.x;
    const uint64_t b0 = log_off[log], b1 = log_off[log + 1];
    if (b1 < b0 || b1 > n_ops || (log == 0 && b0 != 0) || (log + 1 == gridDim.x && b1 != n_ops)) {
        /* offsets that decrease or leave the columns (a wrapped device batch is not checked on the host): no row is touched */
        if (threadIdx.x == 0) {
            atomicOr(&shape[2], 1u);
            need_per_log[log] = 0;
        }
        return;
    }
    if (compute) {
        if (threadIdx.x < 9) sh[threadIdx.x] = 0;
        __syncthreads();
        uint32_t c[6] = {0, 0, 0, 0, 0, 0}, mc = 0, ma = 0, mid = 0;
        for (uint64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x) {
            const uint64_t id = op_id[i];
            const uint32_t a = action[i], mt = mark_type[i];
            mc = max(mc, (uint32_t)(id >> 32));
            ma = max(ma, (uint32_t)id);
            c[0] += a == PTX_ACT_INSERT;
            c[1] += a == PTX_ACT_DELETE;
            const bool mk = a == PTX_ACT_ADDMARK || a == PTX_ACT_REMOVEMARK;
            c[2] += mk && mt == 0;
            c[3] += mk && mt == 1;
            c[4] += mk && mt == 2;
            c[5] += mk && mt == 3;
            if (mk && mt == PTX_MARK_COMMENT) { /* the document's comment-id space as this log has seen it */
                const uint32_t pl = payload[i];
                mid = max(mid, pl == 0xFFFFFFFFu ? pl : pl + 1u);
            }
        }
        for (int k = 0; k < 6; ++k) {
            uint32_t v = c[k];
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[k], v);
        }
        for (int d = 32; d >= 1; d >>= 1) {
            mc = max(mc, (uint32_t)__shfl_xor((int)mc, d, 64));
            ma = max(ma, (uint32_t)__shfl_xor((int)ma, d, 64));
            mid = max(mid, (uint32_t)__shfl_xor((int)mid, d, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMax(&sh[6], mc);
            atomicMax(&sh[7], ma);
            atomicMax(&sh[8], mid);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            ptx_log_hdr h;
            h.n_ins = sh[0];
            h.n_del = sh[1];
            h.n_mark[0] = sh[2];
            h.n_mark[1] = sh[3];
            h.n_mark[2] = sh[4];
            h.n_mark[3] = sh[5];
            h.max_counter = sh[6];
            h.max_actor = sh[7];
            h.n_comment_ids = sh[8];
            h.reserved = 0;
            hdr[log] = h;
        }
    }
    /* does the log use the wide envelope column (some seq / dep beyond 16 bits)?  Then only the HBM-staged kernel can admit it */
    if (threadIdx.x == 0) wide = 0;
    __syncthreads();
    if (chg_off && chg_env_hi) {
        const uint64_t es = PTX_ENV_STRIDE(max_actors), e0 = chg_off[log] * es, e1 = chg_off[log + 1] * es;
        uint32_t any = 0;
        for (uint64_t i = e0 + threadIdx.x; i < e1; i += blockDim.x) any |= chg_env_hi[i];
        if (any) atomicOr(&wide, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const ptx_log_hdr h = hdr[log];
        uint64_t need = ptx_lds_need_hdr(b1 - b0, h);
        const uint64_t C = chg_off ? chg_off[log + 1] - chg_off[log] : 0;
        if (chg_off) need = max(need, ptx_lds_need_admission(C, max_actors));
        /* what the LDS kernel refuses whatever the window (16-bit indices, packed words): such a log takes the HBM-staged path (biglog_core.h) */
        const uint64_t K = (uint64_t)h.n_mark[0] + h.n_mark[1] + h.n_mark[2] + h.n_mark[3];
        const uint64_t ks = ((uint64_t)h.max_counter + 1) * ((uint64_t)h.max_actor + 1);
        uint32_t kbits = 0;
        while ((1ull << kbits) < K + 1) ++kbits;
        const bool lds_ok = b1 - b0 <= 65534u && h.n_ins <= 32766u && h.max_counter < (1u << 19) && h.max_actor <= 4095u && (!h.n_mark[PTX_MARK_COMMENT] || h.n_comment_ids <= 65535u) &&
                            ((ks + 1) << kbits) <= 0xFFFFFFFFull && C <= 65533u && !wide;
        if (!lds_ok) need = 0xFFFFFFFFull;
        if (h.n_ins > 32766u) atomicOr(&shape[2], 2u); /* boundary slots 2 rank + side beyond 16 bits: the result carries their high halves (ptx_dresult.refs_hi) */
        need_per_log[log] = (uint32_t)min(need, (uint64_t)0xFFFFFFFFu);
        big_need_per_log[log] = ptx_big_need(b1 - b0, h, C, max_actors, PTX_BIG_TEAM_MAX);
        if (need <= max_lds) { /* the launch shape of the LDS kernel is sized by the logs that take it */
            atomicMax(&shape[0], (uint32_t)need);
            atomicMax(&shape[1], (uint32_t)(b1 - b0));
            atomicMax(&shape[3], (uint32_t)min(ks, (uint64_t)0xFFFFFFFFu)); /* their largest id keyspace: 16-bit keys everywhere allow the lean builds */
        }
    }
}

/* Calibration stream for the HBM-traffic counters (MI355X_MICROARCH.md "HBM": FETCH_SIZE is exact only for some access widths:
 * calibrate on a known byte count in your own access pattern): every op column and envelope column is read exactly once with
 * the element widths the merge kernel uses (8 B / 4 B / 1 B per lane, consecutive lanes on consecutive rows). */
__global__ void __launch_bounds__(256) ptx_calib_stream_kernel(const uint64_t* op_id, const uint64_t* ref_a, const uint64_t* ref_b, const uint32_t* payload, const uint8_t* action,
                                                                const uint8_t* mark_type, const uint8_t* side_a, const uint8_t* side_b, uint64_t n_rows,
                                                                const uint32_t* chg_hdr, const uint16_t* chg_env, uint64_t n_changes, uint32_t max_actors,
                                                                unsigned long long* sum) {
    unsigned long long acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += stride)
        acc += op_id[i] + ref_a[i] + ref_b[i] + payload[i] + action[i] + mark_type[i] + side_a[i] + side_b[i];
    const uint32_t es = PTX_ENV_STRIDE(max_actors);
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_changes; c += stride) {
        acc += chg_hdr[c];
        const uint2* row = (const uint2*)(chg_env + c * es); /* 8 bytes per lane, as the admission pass reads them */
        for (uint32_t b = 0; b < es / 4u; ++b) acc += row[b].x + row[b].y;
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

__global__ void ptx_count_converged_kernel(const ptx_log_result* res, uint32_t n_docs, uint32_t replicas, unsigned long long* out) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    bool same = d < n_docs;
    if (same) {
        const ptx_log_result* r = res + (uint64_t)d * replicas;
        same = r[0].status == PTX_OK;
        for (uint32_t k = 1; k < replicas && same; ++k) same = r[k].status == PTX_OK && r[k].digest[0] == r[0].digest[0] && r[k].digest[1] == r[0].digest[1];
    }
    const unsigned long long m = __ballot(same);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

__global__ void ptx_count_converged_digests_kernel(const uint64_t* dg, uint64_t n_docs, uint32_t replicas, unsigned long long* out) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool same = d < n_docs;
    if (same) {
        const uint64_t* p = dg + d * replicas * 2;
        same = (p[0] | p[1]) != 0; /* {0, 0} = a failed log */
        for (uint32_t k = 1; k < replicas && same; ++k) same = p[2 * k] == p[0] && p[2 * k + 1] == p[1];
    }
    const unsigned long long m = __ballot(same);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

/* rank-major padded blocks of `width` digest pairs -> the counts[r] valid pairs of every rank, back to back */
__global__ void ptx_compact_digests_kernel(const uint64_t* padded, const uint64_t* first, const uint32_t* counts, uint32_t width, uint64_t* out) {
    const uint32_t r = blockIdx.y;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < counts[r] * 2u; i += gridDim.x * blockDim.x) out[first[r] * 2 + i] = padded[(uint64_t)r * width * 2 + i];
}

__global__ void ptx_pack_digests_kernel(const ptx_log_result* res, uint32_t first, uint32_t count, uint64_t* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        dst[2 * i] = res[first + i].digest[0];
        dst[2 * i + 1] = res[first + i].digest[1];
    }
}

/* ---- compact result rows (ABI 7): the merge writes a log's rows at the log's own row offset (capacity = one row per op: no allocation on the device); a
 *      host wants the rows that EXIST — a few dozen per 4K-op log.  (1) offsets: exclusive prefix sums of n_visible / n_spans / n_cintervals over the logs of the
 *      range, by ONE workgroup (a chunk of 1 024 logs per step; a failed log's counts are 0); (2) gather: a wave per log copies its rows to the dense arrays. ---- */
extern "C" __global__ void __launch_bounds__(1024) ptx_result_offsets_kernel(const ptx_log_result* logs, uint32_t first, uint32_t n_logs, uint64_t* off /* [3][n_logs + 1] */) {
    __shared__ uint64_t wsum[3][16];
    __shared__ uint64_t run[3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 3) run[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_logs; c0 += 1024u) {
        const uint32_t l = c0 + threadIdx.x;
        uint64_t v[3] = {0, 0, 0};
        if (l < n_logs) {
            const ptx_log_result r = logs[first + l];
            v[0] = r.n_visible;
            v[1] = r.n_spans;
            v[2] = r.n_cintervals;
        }
        uint64_t incl[3];
        for (int k = 0; k < 3; ++k) {
            uint64_t x = v[k];
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t y = __shfl_up(x, d, 64);
                if ((int)lane >= d) x += y;
            }
            incl[k] = x;
            if (lane == 63u) wsum[k][wave] = x;
        }
        __syncthreads();
        for (int k = 0; k < 3; ++k) {
            uint64_t base = run[k];
            for (uint32_t w = 0; w < wave; ++w) base += wsum[k][w];
            if (l < n_logs) off[(uint64_t)k * (n_logs + 1) + l] = base + incl[k] - v[k];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            uint64_t t = 0;
            for (uint32_t w = 0; w < 16u; ++w) t += wsum[threadIdx.x][w];
            run[threadIdx.x] += t;
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) off[(uint64_t)threadIdx.x * (n_logs + 1) + n_logs] = run[threadIdx.x];
}
extern "C" __global__ void __launch_bounds__(64) ptx_result_compact_kernel(const uint64_t* log_off, const ptx_log_result* logs, uint32_t first, uint32_t n_logs, const uint64_t* off,
                                                                const uint32_t* values, const ptx_span* spans, const ptx_cinterval* cints, uint32_t* dvalues, ptx_span* dspans,
                                                                ptx_cinterval* dcints) {
    const uint32_t l = blockIdx.x;
    if (l >= n_logs) return;
    const ptx_log_result r = logs[first + l];
    const uint64_t b = log_off[first + l];
    const uint64_t ov = off[l], os = off[(uint64_t)(n_logs + 1) + l], oc = off[2ull * (n_logs + 1) + l];
    for (uint32_t i = threadIdx.x; i < r.n_visible; i += 64u) dvalues[ov + i] = values[b + i];
    for (uint32_t i = threadIdx.x; i < r.n_spans; i += 64u) dspans[os + i] = spans[b + i];
    const uint32_t* cs = (const uint32_t*)(cints + b);
    uint32_t* cd = (uint32_t*)(dcints + oc);
    for (uint32_t i = threadIdx.x; i < 3u * r.n_cintervals; i += 64u) cd[i] = cs[i];
}

/* ---- document text (text_core.h): one wave per log of the range computes the log's length in code units and checks its value ids against the string table;
 *      one workgroup scans lengths and span counts into text_off / span_off (in place, a chunk of 1 024 logs per step); one wave per log assembles the text ---- */
extern "C" __global__ void __launch_bounds__(64) ptx_text_length_kernel(PtxTextArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_text_lds[PTX_TEXT_LDS_BYTES];
    if (blockIdx.x < A.n_logs) ptx_text_length_log<64>(A, blockIdx.x, ptx_text_lds);
}
extern "C" __global__ void __launch_bounds__(1024) ptx_text_offsets_kernel(uint64_t* off /* [2][n_logs + 1]: counts in, exclusive prefix sums out */, uint32_t n_logs) {
    __shared__ uint64_t wsum[2][16];
    __shared__ uint64_t run[2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2) run[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_logs; c0 += 1024u) {
        const uint32_t l = c0 + threadIdx.x;
        uint64_t v[2] = {0, 0}, incl[2];
        for (int k = 0; k < 2; ++k) {
            if (l < n_logs) v[k] = off[(uint64_t)k * (n_logs + 1) + l];
            uint64_t x = v[k];
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t y = __shfl_up(x, d, 64);
                if ((int)lane >= d) x += y;
            }
            incl[k] = x;
            if (lane == 63u) wsum[k][wave] = x;
        }
        __syncthreads();
        for (int k = 0; k < 2; ++k) {
            uint64_t base = run[k];
            for (uint32_t w = 0; w < wave; ++w) base += wsum[k][w];
            if (l < n_logs) off[(uint64_t)k * (n_logs + 1) + l] = base + incl[k] - v[k];
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            uint64_t t = 0;
            for (uint32_t w = 0; w < 16u; ++w) t += wsum[threadIdx.x][w];
            run[threadIdx.x] += t;
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) off[(uint64_t)threadIdx.x * (n_logs + 1) + n_logs] = run[threadIdx.x];
}
extern "C" __global__ void __launch_bounds__(64) ptx_text_assemble_kernel(PtxTextArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_text_lds[PTX_TEXT_LDS_BYTES];
    if (blockIdx.x < A.n_logs) ptx_text_assemble_log<64>(A, blockIdx.x, ptx_text_lds);
}

/* ---- find in the assembled text (find_core.h): one wave per log counts the matches; one workgroup scans min(count, cap) into hit_off (the twin of
 *      ptx_text_offsets_kernel, a chunk of 1 024 logs per step); one wave per log lists its first hits in order and maps them to elements ---- */
extern "C" __global__ void __launch_bounds__(64) ptx_find_count_kernel(PtxFindArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_find_lds[PTX_FIND_LDS_BYTES];
    if (blockIdx.x < A.T.n_logs) ptx_find_count_log<64>(A, blockIdx.x, ptx_find_lds);
}
extern "C" __global__ void __launch_bounds__(1024) ptx_find_offsets_kernel(const uint32_t* n_matches, uint32_t cap, uint64_t* hit_off /* [n_logs + 1] */, uint32_t n_logs) {
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t run;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) run = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_logs; c0 += 1024u) {
        const uint32_t l = c0 + threadIdx.x;
        uint64_t v = 0;
        if (l < n_logs) v = n_matches[l] < cap ? n_matches[l] : cap;
        uint64_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d, 64);
            if ((int)lane >= d) x += y;
        }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint64_t base = run;
        for (uint32_t w = 0; w < wave; ++w) base += wsum[w];
        if (l < n_logs) hit_off[l] = base + x - v;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (uint32_t w = 0; w < 16u; ++w) t += wsum[w];
            run += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) hit_off[n_logs] = run;
}
extern "C" __global__ void __launch_bounds__(64) ptx_find_emit_kernel(PtxFindArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_find_lds[PTX_FIND_LDS_BYTES];
    if (blockIdx.x < A.T.n_logs) ptx_find_emit_log<64>(A, blockIdx.x, ptx_find_lds);
}

/* ---- text and span rows of element ranges (slice_core.h): a lane per log plans the prefix block; one wave per log that has a slice writes its element prefix;
 *      a lane per slice clamps, measures and finds its span rows; ptx_text_offsets_kernel scans both counts; one wave per PTX_SLICE_BLOCK code units of OUTPUT
 *      copies; a lane per output row emits the clipped spans ---- */
extern "C" __global__ void __launch_bounds__(256) ptx_slice_plan_kernel(PtxSliceArgs A) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l < A.T.n_logs) ptx_slice_plan_one(A, l);
}
extern "C" __global__ void __launch_bounds__(64) ptx_slice_prefix_kernel(PtxSliceArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_slice_lds[PTX_SLICE_LDS_BYTES];
    if (blockIdx.x < A.T.n_logs) ptx_slice_prefix_log<64>(A, blockIdx.x, ptx_slice_lds);
}
extern "C" __global__ void __launch_bounds__(256) ptx_slice_bounds_kernel(PtxSliceArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < A.n_slices) ptx_slice_bounds_one(A, k); /* (the grid is ceil(n_slices / 256) <= 2^24 blocks: k does not wrap) */
}
extern "C" __global__ void __launch_bounds__(64) ptx_slice_copy_kernel(PtxSliceArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_slice_lds[PTX_SLICE_LDS_BYTES];
    ptx_slice_copy_block<64>(A, blockIdx.x, ptx_slice_lds); /* (a block behind the output's end returns at once) */
}
extern "C" __global__ void __launch_bounds__(256) ptx_slice_span_kernel(PtxSliceArgs A, uint64_t n_rows) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r < n_rows) ptx_slice_span_one(A, r);
}

/* ---- a resident text view (view_core.h): a lane per log plans the prefix of EVERY good log (then ptx_slice_prefix_kernel writes it); per query one wave per log
 *      lists its first hits' positions (find_core.h's position half), a lane per listed hit finds its elements in the resident prefix, and for snippets a lane
 *      per hit writes the window and match_unit; the slice kernels above do the rest ---- */
extern "C" __global__ void __launch_bounds__(256) ptx_view_plan_kernel(PtxSliceArgs A, uint64_t* every_log) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l < A.T.n_logs) ptx_view_plan_one(A, every_log, l);
}
extern "C" __global__ void __launch_bounds__(64) ptx_view_positions_kernel(PtxFindArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_find_lds[PTX_FIND_LDS_PRE]; /* the header, the pattern and the step's units: no tile scan */
    if (blockIdx.x < A.T.n_logs) (void)ptx_find_positions_log<64>(A, blockIdx.x, ptx_find_lds);
}
extern "C" __global__ void __launch_bounds__(256) ptx_view_locate_kernel(PtxViewArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < A.n_hits) ptx_view_locate_one(A, k); /* (the grid is ceil(n_hits / 256) <= 2^24 blocks: k does not wrap) */
}
extern "C" __global__ void __launch_bounds__(256) ptx_view_windows_kernel(PtxViewArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < A.n_hits) ptx_view_windows_one(A, k);
}

/* ---- find and replace on a view (replace_core.h): after the view's own hit passes, one wave per log chooses the greedy non-overlapping hits by pointer doubling
 *      and marks those that cover whole elements; ptx_find_offsets_kernel scans the Changes and the ops; a lane per hit writes the InputOperations ---- */
extern "C" __global__ void __launch_bounds__(64) ptx_replace_select_kernel(PtxReplaceArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t ptx_replace_lds[PTX_REPLACE_LDS_BYTES];
    if (blockIdx.x < A.V.F.T.n_logs) ptx_replace_select_log<64>(A, blockIdx.x, ptx_replace_lds);
}
extern "C" __global__ void __launch_bounds__(256) ptx_replace_emit_kernel(PtxReplaceArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < A.V.n_hits) ptx_replace_emit_one(A, k); /* (the grid is ceil(n_hits / 256) <= 2^24 blocks: k does not wrap) */
}

/* ---- queries by format on a view (markrun_core.h): one wave per log counts the runs of the selector, ptx_text_offsets_kernel scans min(count, cap), one wave per
 *      log lists its first runs, a lane per listed run measures it (and writes the snippet window); for a find inside marks one wave per log counts the hits its
 *      uncapped runs contain, ptx_find_offsets_kernel scans them under the cap, and the same walk compacts them ---- */
extern "C" __global__ void __launch_bounds__(64) ptx_markrun_count_kernel(PtxMarkRunArgs A) {
    if (blockIdx.x < A.n_logs) ptx_markrun_count_log<64>(A, blockIdx.x);
}
extern "C" __global__ void __launch_bounds__(64) ptx_markrun_emit_kernel(PtxMarkRunArgs A) {
    if (blockIdx.x < A.n_logs) ptx_markrun_emit_log<64>(A, blockIdx.x);
}
extern "C" __global__ void __launch_bounds__(256) ptx_markrun_finish_kernel(PtxMarkRunArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < A.n_listed) ptx_markrun_finish_one(A, k); /* (the grid is ceil(n_listed / 256) <= 2^24 blocks: k does not wrap) */
}
extern "C" __global__ void __launch_bounds__(64) ptx_markrun_filter_count_kernel(PtxMarkFilterArgs A) {
    if (blockIdx.x < A.n_logs) ptx_markrun_filter_log<64, false>(A, blockIdx.x);
}
extern "C" __global__ void __launch_bounds__(64) ptx_markrun_filter_emit_kernel(PtxMarkFilterArgs A) {
    if (blockIdx.x < A.n_logs) ptx_markrun_filter_log<64, true>(A, blockIdx.x);
}

/* log_off of a tiled batch: copy k of log l starts at k * n_ops + log_off[l] */
__global__ void ptx_tile_offsets_kernel(const uint64_t* src, uint64_t* dst, uint32_t n_logs, uint32_t copies, uint64_t n_ops) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = (uint64_t)n_logs * copies;
    if (i < total) dst[i] = (i / n_logs) * n_ops + src[i % n_logs];
    if (i == total) dst[i] = (uint64_t)copies * n_ops;
}

/* ------------------------------------------------------------------------------------------------ */
/* host objects                                                                                     */
/* ------------------------------------------------------------------------------------------------ */

/* rows by which the library over-allocates its copies of the envelope columns: the admission pass reads PTX_AC headers /
 * envelope rows of a lane with one wide load each, also at the last change of the batch */
#define PTX_ENV_PAD 8u
#define PTX_LDS_GRANULE 1280u /* bytes: the CU's 160 KB in 128 granules */

static std::atomic<uint64_t> g_ctx_serial{0};
struct ptx_ctx {
    const uint64_t serial = ++g_ctx_serial; /* never reused, unlike the address of a context or the handle of its stream (launch_merge: who wrote a batch's row index) */
    int device = 0;
    hipStream_t stream = nullptr;     /* the stream in use: own_stream, or the caller's (ptx_set_stream) */
    hipStream_t own_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t side = nullptr;       /* the second launch of a split batch (a few logs with a larger LDS window) runs beside the first */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    int cu_count = 0;
    size_t max_lds = 0;
    int force_threads = 0; /* ptx_set_launch_shape: threads per log (0 = the library's choice) */
    int force_lds = 0;     /* ptx_set_launch_shape: LDS window per log (0 = the library's choice) */
    int stop_after = 0;    /* -DPTX_DIAG builds only (ptx_diag_stop_after): truncate the diagnostic kernel after a phase, for per-phase PMC deltas */
    uint32_t flags = 0;
    bool no_lean256 = false; /* PTX_NO_LEAN256 in the environment when the context was made (read once: wants_lean is on every launch's path) */
    float check_replay_ms = 0.f, check_accum_ms = 0.f; /* the last ptx_check_patches (ptx_check_patches_ms) */
    unsigned long long* clocks = nullptr; /* device [PTX_NCLK], non-null only while ptx_merge_phase_cycles runs */
    /* staging of the SMALL result downloads (an editor session reads one replica per flush): a device block and a pinned host block that the context keeps and
     * grows on demand — a hipMalloc / hipFree (a device-wide wait) / hipHostMalloc / hipHostFree per read cost more than the read */
    uint8_t* stage_d = nullptr;
    uint8_t* stage_h = nullptr;
    size_t stage_d_cap = 0, stage_h_cap = 0;
    uint8_t* up_h = nullptr; /* pinned staging of the small UPLOADS of a call (ptx_change: the InputOperation columns of an edit go up as one copy, not ten) */
    size_t up_h_cap = 0;
    /* freed device blocks of up to PTX_POOL_MAX_BLOCK bytes, by size class (ptx_dev_malloc / ptx_dev_free below) */
    std::map<size_t, std::vector<void*>> pool_free;
    size_t pool_cached = 0;
};

/* ---- small device blocks are KEPT by the context that freed them (round 6, last session) ----
 * An editor session's change() / read is a dozen kernels over a few kilobytes — and was ~80 hipMalloc / hipFree pairs (result buffers, the InputOperation columns, the
 * made batch, the appended batch, offsets, statuses), each a driver call of several microseconds, hipFree a device-wide wait on top: most of the 0.6 ms an edit took.
 * Blocks of up to PTX_POOL_MAX_BLOCK bytes are now handed out in size classes and, when freed, go to a free list of the context whose call frees them (up to
 * PTX_POOL_CAP bytes; the rest, and every larger block — a batch's columns — is hipMalloc / hipFree as before).  A block is only ever reused by calls on the same
 * context, i.e. behind everything that context has put on its stream (the side stream of a split launch is joined before launch_merge returns); ptx_destroy
 * releases them.  Which context a call belongs to: the one its entry point named (ptx_enter), per thread. */
#define PTX_POOL_MAX_BLOCK (4ull << 20)
#define PTX_POOL_CAP (256ull << 20)
struct PtxPoolEntry {
    size_t cls;
    ptx_ctx* owner;
};
static std::mutex g_pool_mu;
static std::unordered_map<void*, PtxPoolEntry> g_pool_live; /* pooled blocks in use */
static std::set<ptx_ctx*> g_pool_ctxs;                      /* contexts alive */
static thread_local ptx_ctx* g_tl_ctx = nullptr;
static size_t ptx_pool_class(size_t bytes) {
    if (bytes <= 4096) return (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    size_t c = 8192;
    while (c < bytes) c <<= 1;
    return c;
}
static hipError_t ptx_dev_malloc(void** p, size_t bytes) {
    if (bytes <= PTX_POOL_MAX_BLOCK && g_tl_ctx) {
        const size_t cls = ptx_pool_class(bytes);
        ptx_ctx* c = nullptr;
        {
            std::lock_guard<std::mutex> g(g_pool_mu);
            if (g_pool_ctxs.count(g_tl_ctx)) {
                c = g_tl_ctx;
                auto it = c->pool_free.find(cls);
                if (it != c->pool_free.end() && !it->second.empty()) {
                    *p = it->second.back();
                    it->second.pop_back();
                    c->pool_cached -= cls;
                    g_pool_live[*p] = PtxPoolEntry{cls, c};
                    return hipSuccess;
                }
            }
        }
        if (c) {
            hipError_t e = hipMalloc(p, cls);
            if (e == hipErrorOutOfMemory) { /* the device is full: what this context keeps goes back first */
                (void)hipGetLastError();
                std::vector<void*> drop;
                {
                    std::lock_guard<std::mutex> g(g_pool_mu);
                    for (auto& kv : c->pool_free) drop.insert(drop.end(), kv.second.begin(), kv.second.end());
                    c->pool_free.clear();
                    c->pool_cached = 0;
                }
                for (void* q : drop) (void)hipFree(q);
                e = hipMalloc(p, cls);
            }
            if (e == hipSuccess) {
                std::lock_guard<std::mutex> g(g_pool_mu);
                g_pool_live[*p] = PtxPoolEntry{cls, c};
            }
            return e;
        }
    }
    return hipMalloc(p, bytes);
}
static hipError_t ptx_dev_free(void* p) {
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        auto it = g_pool_live.find(p);
        if (it != g_pool_live.end()) {
            const PtxPoolEntry en = it->second;
            g_pool_live.erase(it);
            ptx_ctx* c = g_tl_ctx;
            /* kept only by the context that handed it out and in whose call it is freed: its next user then runs behind this context's stream */
            if (c && c == en.owner && g_pool_ctxs.count(c) && c->pool_cached + en.cls <= PTX_POOL_CAP) {
                c->pool_free[en.cls].push_back(p);
                c->pool_cached += en.cls;
                return hipSuccess;
            }
        }
    }
    return hipFree(p);
}
static hipError_t ptx_enter(ptx_ctx* ctx) { /* every entry point that names a context: its device, and the context whose blocks this thread's calls take and return */
    g_tl_ctx = ctx;
    return hipSetDevice(ctx->device);
}

struct ptx_dbatch {
    uint32_t n_logs = 0;
    uint64_t n_ops = 0;
    bool owns = true;
    uint64_t *log_off = nullptr, *op_id = nullptr, *ref_a = nullptr, *ref_b = nullptr;
    uint32_t* payload = nullptr;
    uint8_t *action = nullptr, *mark_type = nullptr, *side_a = nullptr, *side_b = nullptr;
    ptx_log_hdr* log_hdr = nullptr; /* always owned: provided headers are copied, missing ones computed */
    /* Change envelope for causal admission (owned copies; null when the batch came without it) */
    uint64_t* chg_off = nullptr;
    uint32_t* chg_hdr = nullptr;
    uint16_t* chg_env = nullptr;
    uint16_t* chg_env_hi = nullptr; /* the wide column (high halves of chg_env's values), only when some value of the batch needs it */
    uint32_t max_actors = 0;
    uint64_t n_changes = 0;
    /* admission marks (merge_core.h ptx_adm_mark), one 16-byte record per log: what the merge kernel's P0 has admitted of the log so far.  Only a batch that owns
     * its columns and carries the envelope has them (the columns of such a batch never change: what was admitted stays admitted); the one piece of a batch that
     * a merge WRITES — zeroed when the batch is made, freed with it */
    ptx_adm_mark* adm_marks = nullptr;
    /* the row index (merge_core.h ptx_row_index_off): what the merge kernel's row pass P1 derives from op_id / action / mark_type and the headers, kept so that
     * only the FIRST merge of the batch classifies and checks the rows.  Only a batch that owns its columns and whose every LDS-kernel log has 16-bit id keys
     * has one; the big block is never zeroed (rows_indexed, one word per log, says which logs' regions hold anything).  Beside the marks the second thing a
     * merge writes into a batch.  Who writes and who may read is decided per launch (launch_merge) from the state below, under g_index_mu. */
    uint32_t *row_index = nullptr, *row_index_bits = nullptr, *rows_indexed = nullptr;
    /* the operand words of the mark ops (merge_core.h ptx_mark_operand_pack): what P5a derives from ref_a / ref_b / side_a / side_b / payload of a mark op's row,
     * 8 bytes per row of capacity at the index's own region offsets, and one word per log that says whether the log's words stand.  Made with the index or not
     * at all, written by the index's one writer, read by its readers; neither block nullptr or both */
    uint64_t* mark_ops = nullptr;
    uint32_t* mark_ops_stand = nullptr;
    /* the order words (merge_core.h ptx_order_word): what P3 derives from op_id / ref_a / action and the headers — per element its row and its document position,
     * 4 bytes per row of capacity at the index's own region offsets, the tombstone bitmaps addressed like row_index_bits, and one word per log that says whether
     * the log's words stand.  Made with the operand words or not at all (all three nullptr or none), written by the index's one writer, read by its readers */
    uint32_t *order_words = nullptr, *order_bits = nullptr, *order_stands = nullptr;
    mutable int index_state = 0;               /* 0 nobody has written it; 1 a launch is being enqueued that writes it; 2 written by a launch of context index_writer on index_stream, index_ev recorded behind it; 3 that launch has ended */
    mutable uint64_t index_writer = 0;         /* ptx_ctx::serial of the writing context */
    mutable hipStream_t index_stream = nullptr;
    mutable hipEvent_t index_ev = nullptr;
    /* launch shape derived from the largest log */
    uint32_t max_log_ops = 0;
    uint32_t lds_bytes = 0;
    uint32_t threads = 0;
    bool small_keys = false; /* every log the LDS kernel takes has an id keyspace of at most 2^16 (census): the lean builds apply */
    bool wide_slots = false; /* some log has more than 32 766 list elements (census): boundary slots beyond 16 bits — results of this batch carry refs_hi */
    /* split launch: when a few logs need more LDS than the rest, they would cost EVERY log a share of the CU (the
     * dynamic LDS size is per launch): the logs are then merged in two launches, `log_index` = the logs of the main
     * group followed by the rest */
    uint32_t* log_index = nullptr;
    uint32_t n_main = 0;     /* 0 = one launch over all logs */
    uint32_t lds_main = 0;
    /* logs beyond one CU's LDS (biglog_core.h): the last n_big entries of log_index, each with its slice of `big_scratch` (one merge of this batch at a time) */
    uint32_t n_big = 0;
    uint64_t* big_off = nullptr;  /* device [n_big + 1] */
    uint8_t* big_scratch = nullptr;
    /* the LAST n_big_grid of them have at least PTX_BIG_GRID_ROWS rows: each is merged by the workgroups of a cooperative launch of its own (big_grid_wgs[k] of them) */
    uint32_t n_big_grid = 0;
    std::vector<uint32_t> big_grid_wgs;
    uint32_t* grid_bars = nullptr; /* device [2 * n_big_grid]: the grid barriers' words */
};

struct ptx_dresult {
    uint32_t n_logs = 0;
    uint64_t n_rows = 0;
    ptx_log_result* logs = nullptr;
    uint32_t* values = nullptr;
    ptx_span* spans = nullptr;
    ptx_cinterval* cints = nullptr;
    uint32_t* rank = nullptr;
    uint32_t* refs = nullptr; /* with rank: resolved references of the delete / mark rows (PtxMergeArgs.out_refs), for ptx_replay_patches */
    uint32_t* refs_hi = nullptr; /* with refs, for a batch that holds a log of more than 32 766 list elements: the high halves of its mark rows' boundary slots */
};

/* InputOperations resident in HBM (ptx_input_ops_upload / _wrap_device / ptx_view_replace_plan_device): the columns of ptx_input_ops as device pointers, and
 * the sizes the host cannot read off them.  A column is NULL where the caller's was (ptx_change_device refuses what ptx_change refuses) */
struct ptx_dinput_ops {
    uint32_t n_logs = 0, max_actors = 0;
    uint64_t n_changes = 0, n_input_ops = 0, n_values = 0;
    bool owns = true;                              /* false: ptx_input_ops_wrap_device, the columns are the caller's */
    void* blocks[3] = {nullptr, nullptr, nullptr}; /* owned device blocks the pointers below point into */
    uint64_t *chg_off = nullptr, *op_off = nullptr;
    uint8_t *action = nullptr, *mark_type = nullptr;
    uint32_t *index = nullptr, *count = nullptr, *payload = nullptr, *values = nullptr, *actor = nullptr;
};

static std::mutex g_index_mu;                        /* the index_state / index_stream / index_ev of every batch */
static void free_order_words(ptx_dbatch* b) {
    (void)ptx_dev_free(b->order_words);
    (void)ptx_dev_free(b->order_bits);
    (void)ptx_dev_free(b->order_stands);
    b->order_words = b->order_bits = b->order_stands = nullptr;
}
static void free_mark_ops(ptx_dbatch* b) {
    free_order_words(b);
    (void)ptx_dev_free(b->mark_ops);
    (void)ptx_dev_free(b->mark_ops_stand);
    b->mark_ops = nullptr;
    b->mark_ops_stand = nullptr;
}
static void free_row_index(ptx_dbatch* b) {
    free_mark_ops(b);
    (void)ptx_dev_free(b->row_index);
    (void)ptx_dev_free(b->row_index_bits);
    (void)ptx_dev_free(b->rows_indexed);
    b->row_index = b->row_index_bits = b->rows_indexed = nullptr;
    if (b->index_ev) (void)hipEventDestroy(b->index_ev);
    b->index_ev = nullptr;
    b->index_state = 0;
}

static thread_local std::string g_create_err;

static ptx_status fail(ptx_ctx* ctx, ptx_status st, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_err = msg;
    return st;
}

#define PTX_HIP(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t _e = (call);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP,                 \
                        std::string(#call) + ": " + hipGetErrorString(_e));                         \
        }                                                                                           \
    } while (0)

static void shape_launch(ptx_ctx* ctx, ptx_dbatch* b, uint64_t need, uint32_t max_log_ops) {
    b->max_log_ops = max_log_ops;
    uint64_t lds = std::min<uint64_t>(std::max<uint64_t>(need, 4096), ctx->max_lds);
    if (ctx->force_lds) lds = (uint64_t)ctx->force_lds;
    b->lds_bytes = (uint32_t)lds;
    /* threads per log, measured on MI355X (profiles/): fewer waves per log = fewer per-wave fixed costs, more logs per CU;
     * 256-op logs peak at 64 threads, 1K and 2K at 128, 4K at 192, 6K and 8K at 256 (round 4, profiles/r04_i_*: config #5's 8 192-op logs, four per CU by
     * their LDS, run 8 % faster as four waves each than as eight — 74.2 against 68.4 G ops/s; five waves are always the worst choice) */
    uint32_t t = max_log_ops <= 512 ? 64u : max_log_ops <= 2048 ? 128u : max_log_ops <= 4608 ? 192u : max_log_ops <= 12288 ? 256u : 512u;
    /* (round 6) logs of up to 4 608 rows whose window leaves room for six of them or fewer per CU — documents that KEEP their text: thousands of elements — run as
     * four waves each: the wave slots are there, and the tail phases of such a log (LWW trees tile by tile, spans) are work per visible character
     * (`rich4k`, 3 x 4 096 ops at 55 % inserts, five logs per CU: 6.85 against 7.58 ms; 320 threads and more are slower again) */
    if (t == 192u && lds > (160u * 1024u) / 7u) t = 256u;
    if (ctx->force_threads) t = (uint32_t)ctx->force_threads;
    b->threads = t;
}

/* Census of a resident batch: headers (computed on the device unless the caller supplied them) and the
 * launch shape.  `have_hdr`: b->log_hdr already holds the caller's headers. */
static ptx_status census_and_shape(ptx_ctx* ctx, ptx_dbatch* b, bool have_hdr, bool want_index = true /* false: a batch that is merged once (ptx_apply_materialize) */) {
    if (b->owns && b->chg_off && b->n_logs && !b->adm_marks) { /* every batch the library makes comes through here once: nothing of it is admitted yet (an append has copied its base's marks before) */
        hipError_t e = ptx_dev_malloc((void**)&b->adm_marks, (size_t)b->n_logs * sizeof(ptx_adm_mark));
        if (e == hipSuccess) e = hipMemsetAsync(b->adm_marks, 0, (size_t)b->n_logs * sizeof(ptx_adm_mark), ctx->stream);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("admission marks: ") + hipGetErrorString(e));
    }
    uint32_t *shape = nullptr, *d_need = nullptr;
    uint64_t* d_big = nullptr;
    uint32_t h[4] = {0, 0, 0, 0};
    std::vector<uint32_t> need;
    std::vector<uint64_t> big_need;
    if (b->n_logs) {
        PTX_HIP(ctx, ptx_dev_malloc((void**)&shape, 16));
        hipError_t e = ptx_dev_malloc((void**)&d_need, (size_t)b->n_logs * 4);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_big, (size_t)b->n_logs * 8);
        if (e == hipSuccess) e = hipMemsetAsync(shape, 0, 16, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_census_kernel, dim3(b->n_logs), dim3(256), 0, ctx->stream, b->log_off, b->op_id, b->action, b->mark_type, b->payload, b->log_hdr,
                               shape, have_hdr ? 0 : 1, b->chg_off, b->max_actors, d_need, b->n_ops, d_big, (uint32_t)ctx->max_lds, b->chg_env_hi);
            e = hipGetLastError();
        }
        need.resize(b->n_logs);
        big_need.resize(b->n_logs);
        if (e == hipSuccess) e = hipMemcpyAsync(h, shape, 16, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(need.data(), d_need, (size_t)b->n_logs * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(big_need.data(), d_big, (size_t)b->n_logs * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)ptx_dev_free(shape);
        (void)ptx_dev_free(d_need);
        (void)ptx_dev_free(d_big);
        if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("census: ") + hipGetErrorString(e));
        if (h[2] & 1u) return fail(ctx, PTX_ERR_INVALID_ARG, "log_off must run from 0 to n_ops without decreasing");
    }
    shape_launch(ctx, b, h[0], h[1]);
    b->small_keys = h[3] <= 65536u;
    b->wide_slots = (h[2] & 2u) != 0u;
    (void)ptx_dev_free(b->log_index);
    (void)ptx_dev_free(b->big_off);
    (void)ptx_dev_free(b->big_scratch);
    b->log_index = nullptr;
    b->big_off = nullptr;
    b->big_scratch = nullptr;
    b->n_main = 0;
    b->n_big = 0;
    /* Three groups of logs: (1) the many, merged by the LDS kernel at the launch's window; (2) a few that need a larger window — they would cost EVERY log
     * a share of the CU (the dynamic LDS size is per launch), so they get a launch of their own when they are at most a tenth; (3) logs beyond one CU's LDS
     * or the LDS kernel's 16-bit indices: the HBM-staged kernel (biglog_core.h), each with a slice of scratch.  A forced window (ptx_set_launch_shape) keeps
     * (1) and (2) together; a log it does not hold is that log's PTX_ERR_CAPACITY, as documented there. */
    std::vector<uint32_t> big, small;
    for (uint32_t l = 0; l < b->n_logs; ++l) (need[l] > ctx->max_lds && !ctx->force_lds ? big : small).push_back(l);
    (void)ptx_dev_free(b->grid_bars);
    b->grid_bars = nullptr;
    b->n_big_grid = 0;
    b->big_grid_wgs.clear();
    if (!big.empty()) { /* the largest of them get a cooperative launch each (several workgroups per log): they go last */
        std::vector<uint64_t> loff((size_t)b->n_logs + 1);
        hipError_t e = hipMemcpyAsync(loff.data(), b->log_off, ((size_t)b->n_logs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("census (log_off): ") + hipGetErrorString(e));
        auto rows_of = [&](uint32_t l) { return loff[l + 1] - loff[l]; };
        std::stable_partition(big.begin(), big.end(), [&](uint32_t l) { return rows_of(l) < PTX_BIG_GRID_ROWS; });
        for (uint32_t l : big)
            if (rows_of(l) >= PTX_BIG_GRID_ROWS) {
                uint64_t wgs = std::min<uint64_t>(std::max<uint64_t>(rows_of(l) / 1024, 8), PTX_BIG_GRID_MAX_WGS); /* (measured, profiles/r05_e_*: the 100 000-op essay 1.58 / 1.02 / 0.91 ms at 16 / 32 / 64 workgroups) */
                if (const char* ev = getenv("PTX_BIG_GRID_WGS")) wgs = std::min<uint64_t>(std::max<long>(atol(ev), 1), PTX_BIG_GRID_MAX_WGS); /* (tuning runs) */
                b->big_grid_wgs.push_back((uint32_t)wgs);
            }
        b->n_big_grid = (uint32_t)b->big_grid_wgs.size();
        if (b->n_big_grid) {
            e = ptx_dev_malloc((void**)&b->grid_bars, (size_t)b->n_big_grid * 8);
            if (e != hipSuccess) return fail(ctx, PTX_ERR_OOM, "no device memory for the grid barriers");
        }
    }
    uint32_t fit = 0, max_fit = 0;
    bool split = false;
    if (small.size() >= 64 && !ctx->force_lds && b->lds_bytes >= 4096) {
        /* Would one more log fit a CU if the launch were sized for all but a few logs?  The CU hands out LDS in granules of PTX_LDS_GRANULE bytes (measured:
         * tools/micro/occupancy_query.hip, profiles/r03_n_*); k logs share a CU when each needs at most floor(LDS / k) rounded down to a granule. */
        const uint64_t gran = PTX_LDS_GRANULE, lds_now = (b->lds_bytes + gran - 1) / gran * gran;
        const uint64_t k_now = std::max<uint64_t>(ctx->max_lds / lds_now, 1);
        const uint64_t bound = ctx->max_lds / (k_now + 1) / gran * gran; /* per-log LDS at which k_now + 1 logs share a CU */
        for (uint32_t l : small)
            if (need[l] <= bound) {
                ++fit;
                max_fit = std::max(max_fit, need[l]);
            }
        split = fit < small.size() && (uint64_t)fit * 10 >= (uint64_t)small.size() * 9 && k_now < 16;
        if (split) {
            std::stable_partition(small.begin(), small.end(), [&](uint32_t l) { return need[l] <= bound; });
            b->lds_main = (uint32_t)std::max<uint64_t>(max_fit, 4096);
        }
    }
    if (split || !big.empty()) {
        std::vector<uint32_t> idx(small);
        idx.insert(idx.end(), big.begin(), big.end());
        hipError_t e = ptx_dev_malloc((void**)&b->log_index, std::max<size_t>(idx.size(), 1) * 4);
        if (e == hipSuccess && !idx.empty()) e = hipMemcpyAsync(b->log_index, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, ctx->stream);
        b->n_main = split ? fit : (uint32_t)small.size();
        b->n_big = (uint32_t)big.size();
        if (!split) b->lds_main = b->lds_bytes;
        if (e == hipSuccess && !big.empty()) {
            std::vector<uint64_t> off(big.size() + 1, 0);
            for (size_t k = 0; k < big.size(); ++k) off[k + 1] = off[k] + ((big_need[big[k]] + 255) & ~255ull);
            e = ptx_dev_malloc((void**)&b->big_off, off.size() * 8);
            if (e == hipSuccess) e = hipMemcpyAsync(b->big_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = ptx_dev_malloc((void**)&b->big_scratch, std::max<uint64_t>(off.back(), 256));
            if (e == hipErrorOutOfMemory) {
                (void)hipStreamSynchronize(ctx->stream);
                return fail(ctx, PTX_ERR_OOM, "no device memory for the working set of the logs beyond one CU's LDS");
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("launch groups: ") + hipGetErrorString(e));
    }
    /* the row index of a batch that owns its columns: ~4.1 bytes per row beside the 32 of the op log; an allocation that fails leaves the batch without one
     * (every merge then classifies its rows, as before), never with an error.  Only the word per log is zeroed. */
    if (want_index && b->owns && b->n_logs && b->small_keys && !b->rows_indexed) {
        hipError_t e = ptx_dev_malloc((void**)&b->rows_indexed, (size_t)b->n_logs * 4);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&b->row_index, (size_t)ptx_row_index_words(b->n_ops, b->n_logs) * 4);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&b->row_index_bits, (size_t)ptx_row_bits_words(b->n_ops, b->n_logs) * 4);
        if (e == hipSuccess) e = hipMemsetAsync(b->rows_indexed, 0, (size_t)b->n_logs * 4, ctx->stream);
        if (e == hipSuccess) {
            /* the operand words: 8 bytes per row beside the index's ~4.1; a failed allocation leaves the batch with its index and without them, never with an error */
            hipError_t eo = ptx_dev_malloc((void**)&b->mark_ops_stand, (size_t)b->n_logs * 4);
            if (eo == hipSuccess) eo = ptx_dev_malloc((void**)&b->mark_ops, (size_t)ptx_row_index_words(b->n_ops, b->n_logs) * 8);
            if (eo == hipSuccess) eo = hipMemsetAsync(b->mark_ops_stand, 0, (size_t)b->n_logs * 4, ctx->stream);
            if (eo != hipSuccess) {
                (void)hipGetLastError();
                free_mark_ops(b);
            } else {
                /* the order words: 4 bytes per row and a bit per row more; a failed allocation leaves the batch with its operand words and without them,
                 * never with an error.  Only the word per log is zeroed */
                hipError_t er = ptx_dev_malloc((void**)&b->order_stands, (size_t)b->n_logs * 4);
                if (er == hipSuccess) er = ptx_dev_malloc((void**)&b->order_words, (size_t)ptx_row_index_words(b->n_ops, b->n_logs) * 4);
                if (er == hipSuccess) er = ptx_dev_malloc((void**)&b->order_bits, (size_t)ptx_row_bits_words(b->n_ops, b->n_logs) * 4);
                if (er == hipSuccess) er = hipMemsetAsync(b->order_stands, 0, (size_t)b->n_logs * 4, ctx->stream);
                if (er != hipSuccess) {
                    (void)hipGetLastError();
                    free_order_words(b);
                }
            }
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->index_ev, hipEventDisableTiming); /* recorded behind the one merge that writes the index (launch_merge) */
        /* the zeroes stand before the batch is handed out: its first merge may come from another context, on a stream nothing orders behind this one */
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            free_row_index(b);
        }
    }
    return PTX_OK;
}

/* would the LDS window let more than 24 waves share a CU?  Then the build of the merge kernel that fits 7 waves per SIMD (PTX_SGPRS_W7) */
static bool wants_w7(const ptx_ctx* ctx, const ptx_dbatch* b, uint32_t lds) {
    const uint32_t waves = (b->threads + 63u) / 64u, by_lds = (uint32_t)(ctx->max_lds / ((((uint64_t)lds + PTX_LDS_GRANULE - 1u) / PTX_LDS_GRANULE) * PTX_LDS_GRANULE));
    return by_lds * waves > 24u;
}

/* the main launch of a batch through a lean build (see PTX_MERGE_KERNEL_L above)?  0, or its threads per log */
static uint32_t wants_lean(const ptx_ctx* ctx, const ptx_dbatch* b, bool with_rank, uint32_t lds) {
    const bool admit = b->chg_off && !(ctx->flags & PTX_FLAG_NO_ADMISSION);
    if (with_rank || !b->small_keys || ctx->clocks || ctx->stop_after || (admit && b->max_actors > 3)) return 0u;
    if (b->threads == 256u && !ctx->no_lean256) return 256u; /* (whatever the window allows: no register cap in that build) */
    if (!wants_w7(ctx, b, lds)) return 0u;
    return b->threads == 64u || b->threads == 128u || b->threads == 192u ? b->threads : 0u;
}

static ptx_status check_batch(ptx_ctx* ctx, const ptx_batch* h) {
    if (!h) return fail(ctx, PTX_ERR_INVALID_ARG, "batch is NULL");
    if (h->n_logs && !h->log_off) return fail(ctx, PTX_ERR_INVALID_ARG, "log_off is NULL");
    if (h->n_ops && (!h->op_id || !h->ref_a || !h->ref_b || !h->payload || !h->action || !h->mark_type || !h->side_a || !h->side_b))
        return fail(ctx, PTX_ERR_INVALID_ARG, "an op column is NULL");
    return PTX_OK;
}

/* offsets of a HOST batch: start at 0, never decrease, end at the row / change count (the kernels index the columns and
 * the result rows with them) */
static ptx_status check_host_offsets(ptx_ctx* ctx, const ptx_batch* h) {
    if (!h->n_logs) return PTX_OK;
    if (h->log_off[0] != 0 || h->log_off[h->n_logs] != h->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "log_off must run from 0 to n_ops");
    for (uint32_t l = 0; l < h->n_logs; ++l)
        if (h->log_off[l + 1] < h->log_off[l]) return fail(ctx, PTX_ERR_INVALID_ARG, "log_off decreases");
    if (h->chg_off && h->chg_hdr && h->chg_env && h->max_actors) {
        if (h->chg_off[0] != 0) return fail(ctx, PTX_ERR_INVALID_ARG, "chg_off must start at 0");
        for (uint32_t l = 0; l < h->n_logs; ++l)
            if (h->chg_off[l + 1] < h->chg_off[l]) return fail(ctx, PTX_ERR_INVALID_ARG, "chg_off decreases");
    }
    return PTX_OK;
}

template <class T>
static hipError_t dalloc(T** p, uint64_t count) {
    return ptx_dev_malloc((void**)p, std::max<uint64_t>(count, 1) * sizeof(T));
}

/* ------------------------------------------------------------------------------------------------ */
/* C ABI                                                                                            */
/* ------------------------------------------------------------------------------------------------ */

extern "C" {

uint32_t ptx_abi_version(void) { return PTX_ABI_VERSION; }

const char* ptx_kernel_name(void) { return "ptx_merge_kernel"; }

const char* ptx_batch_kernel_name(const ptx_ctx* ctx, const ptx_dbatch* b) {
    if (!ctx || !b) return "ptx_merge_kernel";
    const bool admit = b->chg_off && !(ctx->flags & PTX_FLAG_NO_ADMISSION);
    if (admit && b->max_actors > 3) return b->max_actors >= 8u && b->max_actors <= 15u ? "ptx_merge_kernel_many_wide" : "ptx_merge_kernel_many";
    const uint32_t lds = b->log_index ? b->lds_main : b->lds_bytes;
    const uint32_t lean = wants_lean(ctx, b, !(ctx->flags & PTX_FLAG_NO_ELEM_RANK), lds);
    if (lean) return lean == 64u ? "ptx_merge_kernel_lean64" : lean == 128u ? "ptx_merge_kernel_lean128" : lean == 192u ? "ptx_merge_kernel_lean192" : "ptx_merge_kernel_lean256";
    return wants_w7(ctx, b, lds) ? "ptx_merge_kernel_w7" : "ptx_merge_kernel";
}

const char* ptx_last_error(const ptx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

ptx_status ptx_create(int device_ordinal, uint32_t flags, ptx_ctx** out) {
    if (!out) return fail(nullptr, PTX_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, PTX_ERR_NO_DEVICE, std::string("no HIP device visible (") + hipGetErrorString(e) + "); this library has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= count) return fail(nullptr, PTX_ERR_INVALID_ARG, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return fail(nullptr, PTX_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PTX_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    ptx_ctx* ctx = new ptx_ctx();
    ctx->device = device_ordinal;
    ctx->flags = flags;
    ctx->no_lean256 = getenv("PTX_NO_LEAN256") != nullptr;
    ctx->cu_count = prop.multiProcessorCount;
    ctx->max_lds = 160 * 1024;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
        delete ctx;
        return fail(nullptr, PTX_ERR_HIP, "stream/event creation failed");
    }
    ctx->own_stream = ctx->stream;
    /* one workgroup may use the CU's whole 160 KiB of LDS */
    {
        const void* kernels[] = {(const void*)ptx_merge_kernel, (const void*)ptx_merge_kernel_rest, (const void*)ptx_merge_kernel_many, (const void*)ptx_merge_kernel_many_wide, (const void*)ptx_merge_kernel_diag, (const void*)ptx_merge_kernel_w7, (const void*)ptx_merge_kernel_rest_w7, (const void*)ptx_merge_kernel_lean64, (const void*)ptx_merge_kernel_lean128, (const void*)ptx_merge_kernel_lean192, (const void*)ptx_merge_kernel_lean256, (const void*)ptx_replay_kernel, (const void*)ptx_replay_kernel_gwin, (const void*)ptx_replay_kernel_wide, (const void*)ptx_gen_kernel, (const void*)ptx_gen_kernel_r8, (const void*)ptx_change_kernel, (const void*)ptx_cursor_kernel, (const void*)ptx_rootmap_kernel, (const void*)ptx_sync_plan_kernel, (const void*)ptx_accum_kernel};
        e = hipSuccess;
        for (const void* k : kernels)
            if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->max_lds);
    }
    if (e != hipSuccess) {
        std::string m = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e);
        delete ctx;
        return fail(nullptr, PTX_ERR_HIP, m);
    }
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        g_pool_ctxs.insert(ctx);
    }
    *out = ctx;
    return PTX_OK;
}

void ptx_destroy(ptx_ctx* ctx) {
    if (!ctx) return;
    (void)ptx_enter(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->side) {
        (void)hipStreamSynchronize(ctx->side);
        (void)hipStreamDestroy(ctx->side);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    g_tl_ctx = ctx;
    if (ctx->stage_d) (void)ptx_dev_free(ctx->stage_d);
    if (ctx->stage_h) (void)hipHostFree(ctx->stage_h);
    if (ctx->up_h) (void)hipHostFree(ctx->up_h);
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        g_pool_ctxs.erase(ctx);
        for (auto& kv : ctx->pool_free)
            for (void* q : kv.second) (void)hipFree(q);
        ctx->pool_free.clear();
        ctx->pool_cached = 0;
    }
    g_tl_ctx = nullptr;
    delete ctx;
}

ptx_status ptx_set_launch_shape(ptx_ctx* ctx, uint32_t threads_per_log, uint32_t lds_bytes_per_log) {
    if (!ctx) return PTX_ERR_INVALID_ARG;
    if (threads_per_log && (threads_per_log % 64u || threads_per_log > PTX_MAX_THREADS)) return fail(ctx, PTX_ERR_INVALID_ARG, "threads per log: a multiple of 64 up to 1024");
    if (lds_bytes_per_log > ctx->max_lds) return fail(ctx, PTX_ERR_INVALID_ARG, "LDS window beyond the CU's 160 KiB");
    ctx->force_threads = (int)threads_per_log;
    ctx->force_lds = (int)lds_bytes_per_log;
    return PTX_OK;
}

#ifdef PTX_DIAG
/* diagnostic builds only (tools/phase_insts.sh; earlier rounds: tools/rounds2to5/pmc_phases.sh, trunc_sweep.sh; never declared in include/peritext_hip.h, never in the product
 * library): the diagnostic kernel leaves after the phase with stamp index k — its results are then WRONG by design */
ptx_status ptx_diag_stop_after(ptx_ctx* ctx, uint32_t k) {
    if (!ctx) return PTX_ERR_INVALID_ARG;
    ctx->stop_after = (int)k;
    return PTX_OK;
}
#endif

uint32_t ptx_max_ops_per_log(const ptx_ctx* ctx) {
    /* largest N with lds_need(N, worst split) <= LDS; conservative closed form: ~33 B per row */
    const uint64_t lds = ctx ? ctx->max_lds : 160 * 1024;
    uint32_t lo = 0, hi = 65534;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        const uint64_t worst = std::max(ptx_lds_need(mid, mid, 0, 0, 0, 4ull * mid, 0), ptx_lds_need(mid, mid / 3, mid / 3, mid / 3, mid / 3, 4ull * mid, mid / 3));
        if (worst <= lds) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

void ptx_batch_free(ptx_ctx* ctx, ptx_dbatch* b) {
    if (!b) return;
    if (ctx) (void)ptx_enter(ctx);
    if (b->owns) {
        (void)ptx_dev_free(b->log_off);
        (void)ptx_dev_free(b->op_id);
        (void)ptx_dev_free(b->ref_a);
        (void)ptx_dev_free(b->ref_b);
        (void)ptx_dev_free(b->payload);
        (void)ptx_dev_free(b->action);
        (void)ptx_dev_free(b->mark_type);
        (void)ptx_dev_free(b->side_a);
        (void)ptx_dev_free(b->side_b);
    }
    (void)ptx_dev_free(b->log_hdr);
    (void)ptx_dev_free(b->big_off);
    (void)ptx_dev_free(b->big_scratch);
    (void)ptx_dev_free(b->grid_bars);
    (void)ptx_dev_free(b->log_index);
    (void)ptx_dev_free(b->chg_off);
    (void)ptx_dev_free(b->chg_hdr);
    (void)ptx_dev_free(b->chg_env);
    (void)ptx_dev_free(b->chg_env_hi);
    (void)ptx_dev_free(b->adm_marks);
    free_row_index(b);
    delete b;
}

uint32_t ptx_batch_n_logs(const ptx_dbatch* b) { return b ? b->n_logs : 0; }
void ptx_batch_launch_shape(const ptx_dbatch* b, uint32_t* threads, uint32_t* lds_bytes) {
    if (threads) *threads = b ? b->threads : 0;
    if (lds_bytes) *lds_bytes = b ? (b->log_index ? b->lds_main : b->lds_bytes) : 0;
}
uint64_t ptx_batch_n_ops(const ptx_dbatch* b) { return b ? b->n_ops : 0; }
uint64_t ptx_batch_n_changes(const ptx_dbatch* b) { return b && b->chg_off ? b->n_changes : 0; }
uint32_t ptx_batch_max_actors(const ptx_dbatch* b) { return b && b->chg_off ? b->max_actors : 0; }

static ptx_status upload_tiled(ptx_ctx* ctx, const ptx_batch* h, uint32_t copies, ptx_dbatch** out, bool want_index) {
    if (!ctx || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    ptx_status st = check_batch(ctx, h);
    if (st) return st;
    if (copies == 0) return fail(ctx, PTX_ERR_INVALID_ARG, "copies must be >= 1");
    st = check_host_offsets(ctx, h);
    if (st) return st;
    if ((uint64_t)h->n_logs * copies > 0xFFFFFFFFull) return fail(ctx, PTX_ERR_INVALID_ARG, "too many logs");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dbatch* b = new ptx_dbatch();
    b->n_logs = h->n_logs * copies;
    b->n_ops = h->n_ops * copies;
    const uint64_t M = h->n_ops, T = b->n_ops;
#define PTX_TRY(call)                                   \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string m = std::string(#call) + ": " + hipGetErrorString(_e); \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, m); \
        }                                               \
    } while (0)
    PTX_TRY(dalloc(&b->log_off, (uint64_t)b->n_logs + 1));
    PTX_TRY(dalloc(&b->op_id, T));
    PTX_TRY(dalloc(&b->ref_a, T));
    PTX_TRY(dalloc(&b->ref_b, T));
    PTX_TRY(dalloc(&b->payload, T));
    PTX_TRY(dalloc(&b->action, T + PTX_BYTE_PAD));
    PTX_TRY(dalloc(&b->mark_type, T + PTX_BYTE_PAD));
    PTX_TRY(dalloc(&b->side_a, T));
    PTX_TRY(dalloc(&b->side_b, T));
    PTX_TRY(dalloc(&b->log_hdr, (uint64_t)b->n_logs));
    if (h->log_hdr && h->n_logs) {
        PTX_TRY(hipMemcpyAsync(b->log_hdr, h->log_hdr, (size_t)h->n_logs * sizeof(ptx_log_hdr), hipMemcpyHostToDevice, ctx->stream));
        for (uint32_t k = 1; k < copies; ++k)
            PTX_TRY(hipMemcpyAsync(b->log_hdr + (size_t)k * h->n_logs, b->log_hdr, (size_t)h->n_logs * sizeof(ptx_log_hdr), hipMemcpyDeviceToDevice, ctx->stream));
    }
    const bool have_env = h->chg_off && h->chg_hdr && h->chg_env && h->max_actors && h->n_logs;
    if (have_env) {
        const uint64_t NC = h->chg_off[h->n_logs];
        b->max_actors = h->max_actors;
        b->n_changes = NC * copies;
        PTX_TRY(dalloc(&b->chg_off, (uint64_t)b->n_logs + 1));
        const uint64_t ES = PTX_ENV_STRIDE(h->max_actors);
        PTX_TRY(dalloc(&b->chg_hdr, NC * copies + PTX_ENV_PAD)); /* padding: the admission pass reads headers and rows with 16-byte loads */
        PTX_TRY(dalloc(&b->chg_env, (NC * copies + PTX_ENV_PAD) * ES));
        if (h->chg_env_hi) PTX_TRY(dalloc(&b->chg_env_hi, (NC * copies + PTX_ENV_PAD) * ES));
        for (uint32_t k = 0; k < copies && NC; ++k) {
            const hipMemcpyKind kd = k ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
            PTX_TRY(hipMemcpyAsync(b->chg_hdr + k * NC, k ? (const void*)b->chg_hdr : (const void*)h->chg_hdr, NC * 4, kd, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->chg_env + k * NC * ES, k ? (const void*)b->chg_env : (const void*)h->chg_env, NC * ES * 2, kd, ctx->stream));
            if (h->chg_env_hi)
                PTX_TRY(hipMemcpyAsync(b->chg_env_hi + k * NC * ES, k ? (const void*)b->chg_env_hi : (const void*)h->chg_env_hi, NC * ES * 2, kd, ctx->stream));
        }
        uint64_t* tmpc = nullptr;
        PTX_TRY(dalloc(&tmpc, (uint64_t)h->n_logs + 1));
        hipError_t ec = hipMemcpyAsync(tmpc, h->chg_off, ((uint64_t)h->n_logs + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
        if (ec == hipSuccess) {
            const uint64_t total = (uint64_t)b->n_logs + 1;
            hipLaunchKernelGGL(ptx_tile_offsets_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, tmpc, b->chg_off, h->n_logs, copies, NC);
            ec = hipGetLastError();
        }
        hipError_t ec2 = hipStreamSynchronize(ctx->stream);
        (void)ptx_dev_free(tmpc);
        PTX_TRY(ec);
        PTX_TRY(ec2);
    }
    if (M) {
        PTX_TRY(hipMemcpyAsync(b->op_id, h->op_id, M * 8, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->ref_a, h->ref_a, M * 8, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->ref_b, h->ref_b, M * 8, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->payload, h->payload, M * 4, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->action, h->action, M, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->mark_type, h->mark_type, M, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->side_a, h->side_a, M, hipMemcpyHostToDevice, ctx->stream));
        PTX_TRY(hipMemcpyAsync(b->side_b, h->side_b, M, hipMemcpyHostToDevice, ctx->stream));
        for (uint32_t k = 1; k < copies; ++k) { /* replicate inside HBM: distinct addresses per copy */
            PTX_TRY(hipMemcpyAsync(b->op_id + k * M, b->op_id, M * 8, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->ref_a + k * M, b->ref_a, M * 8, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->ref_b + k * M, b->ref_b, M * 8, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->payload + k * M, b->payload, M * 4, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->action + k * M, b->action, M, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->mark_type + k * M, b->mark_type, M, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->side_a + k * M, b->side_a, M, hipMemcpyDeviceToDevice, ctx->stream));
            PTX_TRY(hipMemcpyAsync(b->side_b + k * M, b->side_b, M, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    {
        uint64_t* tmp = nullptr;
        PTX_TRY(dalloc(&tmp, (uint64_t)h->n_logs + 1));
        hipError_t e1 = h->n_logs ? hipMemcpyAsync(tmp, h->log_off, ((uint64_t)h->n_logs + 1) * 8, hipMemcpyHostToDevice, ctx->stream) : hipSuccess; /* an empty batch may come without log_off */
        if (e1 == hipSuccess && h->n_logs) {
            const uint64_t total = (uint64_t)b->n_logs + 1;
            hipLaunchKernelGGL(ptx_tile_offsets_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, tmp, b->log_off,
                               h->n_logs, copies, M);
            e1 = hipGetLastError();
        } else if (e1 == hipSuccess) {
            e1 = hipMemsetAsync(b->log_off, 0, 8, ctx->stream);
        }
        hipError_t e2 = hipStreamSynchronize(ctx->stream);
        (void)ptx_dev_free(tmp);
        PTX_TRY(e1);
        PTX_TRY(e2);
    }
#undef PTX_TRY
    st = census_and_shape(ctx, b, h->log_hdr != nullptr, want_index);
    if (st) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *out = b;
    return PTX_OK;
}

ptx_status ptx_batch_upload_tiled(ptx_ctx* ctx, const ptx_batch* h, uint32_t copies, ptx_dbatch** out) { return upload_tiled(ctx, h, copies, out, true); }
ptx_status ptx_batch_upload(ptx_ctx* ctx, const ptx_batch* host, ptx_dbatch** out) { return upload_tiled(ctx, host, 1, out, true); }

ptx_status ptx_batch_append_device(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_dbatch* m, ptx_dbatch** out) {
    if (!ctx || !base || !m || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    if (m->n_logs != base->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_append: `more` must have the logs of `base` (empty ones allowed)");
    /* a base without a single row has no envelope to speak of: it takes the one of `more` */
    const bool base_env = base->chg_off != nullptr, more_env = m->chg_off != nullptr;
    const bool env = more_env && (base_env || base->n_ops == 0);
    if ((base_env && base->n_ops && !more_env) || (more_env && !env) || (env && base_env && base->n_changes && m->max_actors != base->max_actors))
        return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_append: both batches carry the Change envelope with the same max_actors, or neither does");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dbatch* b = new ptx_dbatch();
    b->n_logs = base->n_logs;
    b->n_ops = base->n_ops + m->n_ops;
    b->max_actors = env ? m->max_actors : 0;
    b->n_changes = env ? (base_env ? base->n_changes : 0) + m->n_changes : 0;
    const uint64_t T = b->n_ops, NC = b->n_changes, L = b->n_logs;
    uint64_t* zero_off = nullptr; /* stands in for the envelope offsets of an envelope-less empty base */
#define PTX_TRYA(call)                                  \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string msg = std::string(#call) + ": " + hipGetErrorString(_e); \
            (void)ptx_dev_free(zero_off);                    \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, msg); \
        }                                               \
    } while (0)
    PTX_TRYA(dalloc(&b->log_off, L + 1));
    PTX_TRYA(dalloc(&b->op_id, T));
    PTX_TRYA(dalloc(&b->ref_a, T));
    PTX_TRYA(dalloc(&b->ref_b, T));
    PTX_TRYA(dalloc(&b->payload, T));
    PTX_TRYA(dalloc(&b->action, T + PTX_BYTE_PAD));
    PTX_TRYA(dalloc(&b->mark_type, T + PTX_BYTE_PAD));
    PTX_TRYA(dalloc(&b->side_a, T));
    PTX_TRYA(dalloc(&b->side_b, T));
    PTX_TRYA(dalloc(&b->log_hdr, L));
    if (env) {
        PTX_TRYA(dalloc(&b->chg_off, L + 1));
        PTX_TRYA(dalloc(&b->chg_hdr, NC + PTX_ENV_PAD));
        PTX_TRYA(dalloc(&b->chg_env, (NC + PTX_ENV_PAD) * PTX_ENV_STRIDE(b->max_actors)));
        if ((base_env && base->chg_env_hi) || m->chg_env_hi) PTX_TRYA(dalloc(&b->chg_env_hi, (NC + PTX_ENV_PAD) * PTX_ENV_STRIDE(b->max_actors)));
        if (!base_env) {
            PTX_TRYA(dalloc(&zero_off, L + 1));
            PTX_TRYA(hipMemsetAsync(zero_off, 0, (L + 1) * 8, ctx->stream));
        }
    }
    if (L) {
        const uint64_t* base_coff = base_env ? base->chg_off : zero_off;
        const unsigned blocks = (unsigned)((L + 1 + 255) / 256);
        hipLaunchKernelGGL(ptx_append_offsets_kernel, dim3(blocks), dim3(256), 0, ctx->stream, base->log_off, m->log_off, b->log_off, (uint32_t)L);
        if (env) hipLaunchKernelGGL(ptx_append_offsets_kernel, dim3(blocks), dim3(256), 0, ctx->stream, base_coff, m->chg_off, b->chg_off, (uint32_t)L);
        PtxAppendCols A = {base->op_id, base->ref_a, base->ref_b, base->payload, base->action, base->mark_type, base->side_a, base->side_b,
                           base->chg_hdr, base->chg_env, base_env ? base->chg_env_hi : nullptr};
        PtxAppendCols B = {m->op_id, m->ref_a, m->ref_b, m->payload, m->action, m->mark_type, m->side_a, m->side_b, m->chg_hdr, m->chg_env, m->chg_env_hi};
        PtxAppendDst D = {b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b, b->chg_hdr, b->chg_env, b->chg_env_hi};
        hipLaunchKernelGGL(ptx_append_rows_kernel, dim3((unsigned)L), dim3(256), 0, ctx->stream, A, base->log_off, env ? base_coff : nullptr, B, m->log_off,
                           env ? m->chg_off : nullptr, D, b->log_off, env ? b->chg_off : nullptr, b->max_actors);
        PTX_TRYA(hipGetLastError());
        PTX_TRYA(hipStreamSynchronize(ctx->stream));
    } else {
        PTX_TRYA(hipMemsetAsync(b->log_off, 0, 8, ctx->stream));
        if (env) PTX_TRYA(hipMemsetAsync(b->chg_off, 0, 8, ctx->stream));
        PTX_TRYA(hipStreamSynchronize(ctx->stream));
    }
    /* what the base's merges have admitted of every log stays admitted: the new log is the old one and more.  (A record holds the clock of up to three actors;
     * a batch of more starts from nothing, as does one whose base has no marks) */
    if (env && L && base_env && base->adm_marks && base->max_actors <= 3u && b->max_actors <= 3u) {
        PTX_TRYA(ptx_dev_malloc((void**)&b->adm_marks, (size_t)L * sizeof(ptx_adm_mark)));
        PTX_TRYA(hipMemcpyAsync(b->adm_marks, base->adm_marks, (size_t)L * sizeof(ptx_adm_mark), hipMemcpyDeviceToDevice, ctx->stream));
    }
#undef PTX_TRYA
    (void)ptx_dev_free(zero_off);
    const ptx_status st = census_and_shape(ctx, b, false);
    if (st != PTX_OK) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *out = b;
    return PTX_OK;
}

ptx_status ptx_batch_append(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_batch* more, ptx_dbatch** out) {
    if (!ctx || !base || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    ptx_status st = check_batch(ctx, more);
    if (st) return st;
    if (more->n_logs != base->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_append: `more` must have the logs of `base` (empty ones allowed)");
    ptx_dbatch* m = nullptr;
    st = ptx_batch_upload(ctx, more, &m);
    if (st) return st;
    st = ptx_batch_append_device(ctx, base, m, out);
    ptx_batch_free(ctx, m);
    return st;
}

ptx_status ptx_batch_wrap_device(ptx_ctx* ctx, const ptx_batch* d, ptx_dbatch** out) {
    if (!ctx || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    ptx_status st = check_batch(ctx, d);
    if (st) return st;
    ptx_dbatch* b = new ptx_dbatch();
    b->owns = false;
    b->n_logs = d->n_logs;
    b->n_ops = d->n_ops;
    b->log_off = (uint64_t*)d->log_off;
    b->op_id = (uint64_t*)d->op_id;
    b->ref_a = (uint64_t*)d->ref_a;
    b->ref_b = (uint64_t*)d->ref_b;
    b->payload = (uint32_t*)d->payload;
    b->action = (uint8_t*)d->action;
    b->mark_type = (uint8_t*)d->mark_type;
    b->side_a = (uint8_t*)d->side_a;
    b->side_b = (uint8_t*)d->side_b;
    PTX_HIP(ctx, ptx_enter(ctx));
    hipError_t e = dalloc(&b->log_hdr, (uint64_t)b->n_logs);
    if (e == hipSuccess && d->log_hdr && b->n_logs)
        e = hipMemcpyAsync(b->log_hdr, d->log_hdr, (size_t)b->n_logs * sizeof(ptx_log_hdr), hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) {
        ptx_batch_free(ctx, b);
        return fail(ctx, PTX_ERR_HIP, std::string("wrap: ") + hipGetErrorString(e));
    }
    st = census_and_shape(ctx, b, d->log_hdr != nullptr);
    if (st) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *out = b;
    return PTX_OK;
}

void ptx_dresult_free(ptx_ctx* ctx, ptx_dresult* r) {
    if (!r) return;
    if (ctx) (void)ptx_enter(ctx);
    (void)ptx_dev_free(r->logs);
    (void)ptx_dev_free(r->values);
    (void)ptx_dev_free(r->spans);
    (void)ptx_dev_free(r->cints);
    (void)ptx_dev_free(r->rank);
    (void)ptx_dev_free(r->refs);
    (void)ptx_dev_free(r->refs_hi);
    delete r;
}

ptx_status ptx_result_alloc(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult** out) {
    if (!ctx || !b || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dresult* r = new ptx_dresult();
    r->n_logs = b->n_logs;
    r->n_rows = b->n_ops;
    hipError_t e = dalloc(&r->logs, r->n_logs);
    if (e == hipSuccess) e = dalloc(&r->values, r->n_rows);
    if (e == hipSuccess) e = dalloc(&r->spans, r->n_rows);
    if (e == hipSuccess) e = dalloc(&r->cints, r->n_rows);
    if (e == hipSuccess && !(ctx->flags & PTX_FLAG_NO_ELEM_RANK)) e = dalloc(&r->rank, r->n_rows);
    if (e == hipSuccess && !(ctx->flags & PTX_FLAG_NO_ELEM_RANK)) e = dalloc(&r->refs, r->n_rows);
    if (e == hipSuccess && !(ctx->flags & PTX_FLAG_NO_ELEM_RANK) && b->wide_slots) e = dalloc(&r->refs_hi, r->n_rows);
    if (e != hipSuccess) {
        std::string m = std::string("result allocation: ") + hipGetErrorString(e);
        ptx_dresult_free(ctx, r);
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, m);
    }
    *out = r;
    return PTX_OK;
}

static ptx_status launch_merge(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r) {
    if (b->n_logs == 0) return PTX_OK;
    PtxMergeArgs A;
    A.log_off = b->log_off;
    A.op_id = b->op_id;
    A.ref_a = b->ref_a;
    A.ref_b = b->ref_b;
    A.payload = b->payload;
    A.action = b->action;
    A.mark_type = b->mark_type;
    A.side_a = b->side_a;
    A.side_b = b->side_b;
    A.log_hdr = b->log_hdr;
    const bool admit = b->chg_off && !(ctx->flags & PTX_FLAG_NO_ADMISSION);
    A.chg_off = admit ? b->chg_off : nullptr;
    A.chg_hdr = b->chg_hdr;
    A.chg_env = b->chg_env;
    A.chg_env_hi = b->chg_env_hi;
    A.max_actors = b->max_actors;
    A.clocks = ctx->clocks;
    A.stop_after = (uint32_t)ctx->stop_after;
    A.res = r->logs;
    A.out_values = r->values;
    A.out_spans = r->spans;
    A.out_cints = r->cints;
    A.out_rank = r->rank;
    A.out_refs = r->refs;
    A.out_refs_hi = r->refs_hi;
    A.n_logs = b->n_logs;
    A.lds_bytes = b->lds_bytes;
    A.div_magic = (uint32_t)(0x100000000ull / b->threads) + 1u;
    A.log_index = nullptr;
    A.big_scratch = b->big_scratch;
    A.big_off = b->big_off;
    A.grid_bar = nullptr;
    /* (the diagnostic launches measure the walk; PTX_FLAG_READMIT asks for it) */
    A.adm_marks = admit && !(ctx->flags & PTX_FLAG_READMIT) && !ctx->clocks && !ctx->stop_after ? b->adm_marks : nullptr;
    /* The row index.  The order of a log's lists differs from launch to launch (their slots come from one LDS atomic per wave), so two launches writing one
     * log's region at once would interleave two permutations: exactly ONE launch per batch ever writes — the first eligible ptx_merge (its main / rest launches
     * write disjoint logs and count as one writer).  A launch READS the index only if it is ordered after the WHOLE kernel that wrote it: a later launch on the
     * writer's stream by stream order, a launch on another stream once hipEventQuery says the event recorded behind the writer has completed.  So what a reader
     * sees was complete before its kernel began, and no argument about visibility between XCDs inside a kernel is needed.  Until then a launch on another
     * stream neither reads nor writes: it parks in its result's span rows, as before — nothing waits.  PTX_FLAG_READMIT and the diagnostic launches stay out
     * altogether, like with the marks. */
    int idx_mode = 0; /* 1 write, 2 read */
    if (b->row_index && !(ctx->flags & PTX_FLAG_READMIT) && !ctx->clocks && !ctx->stop_after) {
        std::lock_guard<std::mutex> g(g_index_mu);
        if (b->index_state == 0) { /* (the event was made with the index: a driver call here would stand between the caller and its first merge) */
            b->index_state = 1;
            b->index_writer = ctx->serial;
            b->index_stream = ctx->stream;
            idx_mode = 1;
        } else if (b->index_state == 2) {
            /* the writing context itself, still on the stream it wrote on (ptx_set_stream drains the stream it leaves): stream order, and no driver call in
             * its launch path.  A context's serial is never reused, so a stream handle that comes back after a context was destroyed cannot pass for it */
            if (b->index_writer == ctx->serial && b->index_stream == ctx->stream) idx_mode = 2;
            else if (hipEventQuery(b->index_ev) == hipSuccess) {
                b->index_state = 3;
                idx_mode = 2;
            } else (void)hipGetLastError(); /* (hipErrorNotReady) */
        } else if (b->index_state == 3) idx_mode = 2;
    }
    A.row_index = idx_mode ? b->row_index : nullptr;
    A.row_index_bits = idx_mode ? b->row_index_bits : nullptr;
    A.rows_indexed = idx_mode ? b->rows_indexed : nullptr;
    A.row_index_write = idx_mode == 1 ? 1u : 0u;
    A.mark_ops = idx_mode ? b->mark_ops : nullptr; /* (with the index, under its protocol: its writer writes them, its readers read them) */
    A.mark_ops_stand = idx_mode ? b->mark_ops_stand : nullptr;
    A.order_checks_once = idx_mode == 2 && b->mark_ops ? 1u : 0u; /* (a reading launch: a log whose word stands passed its row-order checks in the writing launch) */
    A.order_words = idx_mode ? b->order_words : nullptr; /* (with the operand words, under the index's protocol) */
    A.order_bits = idx_mode ? b->order_bits : nullptr;
    A.order_stands = idx_mode ? b->order_stands : nullptr;
    /* one workgroup per log; far more workgroups than the 256 CUs so the dispatcher load-balances.  Up to three launches (census_and_shape): the many at
     * their LDS window, the few that need a larger one, the logs beyond one CU's LDS through the HBM-staged kernel — the latter two on a side stream forked
     * from and joined to the caller's, so that they run beside the many instead of after them. */
    const bool diag = ctx->clocks || ctx->stop_after;
    const uint32_t n_small = b->log_index ? b->n_logs - b->n_big : b->n_logs;
    const uint32_t n_rest = b->log_index ? n_small - b->n_main : 0;
    const bool fork = (n_rest || b->n_big) && !diag && ctx->side;
    if (fork) {
        (void)hipEventRecord(ctx->ev_fork, ctx->stream);
        (void)hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0);
    }
    for (int part = 0; part < 3; ++part) {
        uint32_t grid = part == 0 ? (b->log_index ? b->n_main : b->n_logs) : part == 1 ? n_rest : b->n_big;
        if (grid == 0) continue;
        uint32_t lds = part == 0 && b->log_index ? b->lds_main : b->lds_bytes;
        A.log_index = b->log_index ? b->log_index + (part == 0 ? 0 : part == 1 ? b->n_main : n_small) : nullptr;
        A.n_logs = grid;
        A.lds_bytes = lds;
        hipStream_t st = part && fork ? ctx->side : ctx->stream;
        if (part == 2) {
            const uint32_t n_single = b->n_big - b->n_big_grid; /* one 1 024-thread workgroup each; then the largest logs, a cooperative launch of several workgroups each */
            if (n_single) hipLaunchKernelGGL(ptx_merge_big_kernel, dim3(n_single), dim3(PTX_BIG_THREADS), (uint32_t)ptx_a16(sizeof(PtxHdr)), st, A);
            if (b->n_big_grid) (void)hipMemsetAsync(b->grid_bars, 0, (size_t)b->n_big_grid * 8, st);
            for (uint32_t k = 0; k < b->n_big_grid; ++k) {
                PtxMergeArgs G = A;
                G.log_index = A.log_index + n_single + k;
                G.big_off = b->big_off + n_single + k;
                G.grid_bar = b->grid_bars + 2 * k;
                G.n_logs = 1;
                void* kargs[] = {(void*)&G};
                /* (read per launch of a large log, not once in ptx_create: tests/test_gpu_biglog.py sets it after its context exists, and this loop is not the
                 * hot path — it runs once per log of 16 384 rows and more) */
                hipError_t ce = getenv("PTX_NO_COOPERATIVE") ? hipErrorCooperativeLaunchTooLarge /* (tests: a runtime without cooperative launch) */
                                                               : hipLaunchCooperativeKernel((const void*)ptx_merge_big_grid_kernel, dim3(b->big_grid_wgs[k]), dim3(PTX_BIG_GRID_THREADS), kargs, 0, st);
                if (ce != hipSuccess) {
                    /* no cooperative launch here: the log is merged by ONE workgroup of the HBM-staged kernel — its slice of scratch covers that form too —,
                     * slower, never a failed batch; and the side stream is joined below whatever happens */
                    (void)hipGetLastError();
                    G.grid_bar = nullptr;
                    hipLaunchKernelGGL(ptx_merge_big_kernel, dim3(1), dim3(PTX_BIG_THREADS), (uint32_t)ptx_a16(sizeof(PtxHdr)), st, G);
                }
            }
        }
        else if (diag) { /* + room for its phase stamps in the header */
            A.lds_bytes = std::min<uint32_t>(lds + PTX_HDR_DIAG_EXTRA, (uint32_t)ctx->max_lds);
#ifdef PTX_DIAG
            const bool dl_ok = !part && !(r->rank || r->refs) && b->small_keys && !(admit && b->max_actors > 3) && wants_w7(ctx, b, lds);
            const uint32_t dl = dl_ok && (b->threads == 64u || b->threads == 128u || b->threads == 192u) ? b->threads : 0u;
            if (dl == 64u) hipLaunchKernelGGL(ptx_merge_kernel_diag64, dim3(grid), dim3(64), A.lds_bytes, st, A);
            else if (dl == 128u) hipLaunchKernelGGL(ptx_merge_kernel_diag128, dim3(grid), dim3(128), A.lds_bytes, st, A);
            else if (dl == 192u) hipLaunchKernelGGL(ptx_merge_kernel_diag192, dim3(grid), dim3(192), A.lds_bytes, st, A);
            else
#endif
            hipLaunchKernelGGL(ptx_merge_kernel_diag, dim3(grid), dim3(b->threads), A.lds_bytes, st, A);
        }
        else if (admit && b->max_actors > 3) {
            if (b->max_actors >= 8u && b->max_actors <= 15u) hipLaunchKernelGGL(ptx_merge_kernel_many_wide, dim3(grid), dim3(b->threads), lds, st, A);
            else hipLaunchKernelGGL(ptx_merge_kernel_many, dim3(grid), dim3(b->threads), lds, st, A);
        }
        else {
            const bool w7 = wants_w7(ctx, b, lds);
            const uint32_t lean = part ? 0u : wants_lean(ctx, b, r->rank || r->refs, lds);
            if (part) hipLaunchKernelGGL(w7 ? ptx_merge_kernel_rest_w7 : ptx_merge_kernel_rest, dim3(grid), dim3(b->threads), lds, st, A);
            else if (lean == 64u) hipLaunchKernelGGL(ptx_merge_kernel_lean64, dim3(grid), dim3(64), lds, st, A);
            else if (lean == 128u) hipLaunchKernelGGL(ptx_merge_kernel_lean128, dim3(grid), dim3(128), lds, st, A);
            else if (lean == 192u) hipLaunchKernelGGL(ptx_merge_kernel_lean192, dim3(grid), dim3(192), lds, st, A);
            else if (lean == 256u) hipLaunchKernelGGL(ptx_merge_kernel_lean256, dim3(grid), dim3(256), lds, st, A);
            else hipLaunchKernelGGL(w7 ? ptx_merge_kernel_w7 : ptx_merge_kernel, dim3(grid), dim3(b->threads), lds, st, A);
        }
    }
    if (fork) {
        (void)hipEventRecord(ctx->ev_join, ctx->side);
        (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    }
    if (idx_mode == 1) { /* behind every launch of this merge (the side stream has been joined): from here on others may learn that the index stands */
        std::lock_guard<std::mutex> g(g_index_mu);
        if (hipEventRecord(b->index_ev, ctx->stream) == hipSuccess) b->index_state = 2;
        else (void)hipGetLastError(); /* (state 1 for good: nobody reads, nobody writes again) */
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("ptx_merge_kernel launch: ") + hipGetErrorString(e));
    return PTX_OK;
}

ptx_status ptx_merge(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r) {
    if (!ctx || !b || !r) return PTX_ERR_INVALID_ARG;
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    PTX_HIP(ctx, ptx_enter(ctx));
    return launch_merge(ctx, b, r);
}

/* Test hook, NOT part of the C ABI (no declaration in the header; the GPU suite binds it by name): where the row index of a batch stands.  Returns -1 for a
 * batch without an index, else the host's state (0 nobody has written it .. 3 the writing merge has ended); *n_indexed = the logs whose rows_indexed is set,
 * read after everything this context has enqueued. */
int ptx_debug_row_index(ptx_ctx* ctx, const ptx_dbatch* b, uint32_t* n_indexed) {
    if (n_indexed) *n_indexed = 0;
    if (!ctx || !b || !b->rows_indexed) return -1;
    if (ptx_enter(ctx) != hipSuccess) return -1;
    std::vector<uint32_t> h(b->n_logs);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(h.data(), b->rows_indexed, (size_t)b->n_logs * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n_indexed)
        for (uint32_t v : h) *n_indexed += v != 0u;
    std::lock_guard<std::mutex> g(g_index_mu);
    return b->index_state;
}

/* Test hook beside ptx_debug_row_index, NOT part of the C ABI: *n_stand = the logs whose operand words stand (mark_ops_stand set), read after everything this
 * context has enqueued.  Returns -1 for a batch without operand words, else 0. */
int ptx_debug_mark_operands(ptx_ctx* ctx, const ptx_dbatch* b, uint32_t* n_stand) {
    if (n_stand) *n_stand = 0;
    if (!ctx || !b || !b->mark_ops || !b->mark_ops_stand) return -1;
    if (ptx_enter(ctx) != hipSuccess) return -1;
    std::vector<uint32_t> h(b->n_logs);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(h.data(), b->mark_ops_stand, (size_t)b->n_logs * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n_stand)
        for (uint32_t v : h) *n_stand += v != 0u;
    return 0;
}

/* Test hook beside ptx_debug_mark_operands, NOT part of the C ABI: *n_stand = the logs whose order words stand (order_stands set), read after everything this
 * context has enqueued.  Returns -1 for a batch without order words, else 0. */
int ptx_debug_order_words(ptx_ctx* ctx, const ptx_dbatch* b, uint32_t* n_stand) {
    if (n_stand) *n_stand = 0;
    if (!ctx || !b || !b->order_words || !b->order_stands) return -1;
    if (ptx_enter(ctx) != hipSuccess) return -1;
    std::vector<uint32_t> h(b->n_logs);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(h.data(), b->order_stands, (size_t)b->n_logs * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n_stand)
        for (uint32_t v : h) *n_stand += v != 0u;
    return 0;
}

ptx_status ptx_merge_timed(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r, uint32_t iters, float* ms_total) {
    if (!ctx || !b || !r || !ms_total) return PTX_ERR_INVALID_ARG;
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        ptx_status st = launch_merge(ctx, b, r);
        if (st) return st;
    }
    PTX_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    PTX_HIP(ctx, hipEventSynchronize(ctx->ev1));
    PTX_HIP(ctx, hipEventElapsedTime(ms_total, ctx->ev0, ctx->ev1));
    return PTX_OK;
}

ptx_status ptx_merge_phase_cycles(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r, uint64_t* cycles, uint32_t n) {
    if (!ctx || !b || !r || !cycles) return PTX_ERR_INVALID_ARG;
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    PTX_HIP(ctx, ptx_enter(ctx));
    unsigned long long* d = nullptr;
    PTX_HIP(ctx, ptx_dev_malloc((void**)&d, PTX_NCLK * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, PTX_NCLK * sizeof(unsigned long long), ctx->stream);
    ptx_status st = PTX_OK;
    if (e == hipSuccess) {
        ctx->clocks = d;
        st = launch_merge(ctx, b, r);
        ctx->clocks = nullptr;
    }
    unsigned long long h[PTX_NCLK];
    if (e == hipSuccess && st == PTX_OK) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)ptx_dev_free(d);
    if (st) return st;
    if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("phase cycles: ") + hipGetErrorString(e));
    for (uint32_t k = 0; k < n; ++k) cycles[k] = k < PTX_NCLK ? (uint64_t)h[k] : 0;
    return PTX_OK;
}

ptx_status ptx_set_stream(ptx_ctx* ctx, void* hip_stream) {
    if (!ctx) return PTX_ERR_INVALID_ARG;
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream)); /* nothing of this context is left in flight on the stream it leaves */
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return PTX_OK;
}

ptx_status ptx_count_converged(ptx_ctx* ctx, const ptx_dresult* r, uint32_t replicas, uint64_t* count_device) {
    if (!ctx || !r || !count_device || replicas == 0) return PTX_ERR_INVALID_ARG;
    if (r->n_logs % replicas) return fail(ctx, PTX_ERR_INVALID_ARG, "n_logs is not a multiple of replicas");
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, hipMemsetAsync(count_device, 0, 8, ctx->stream));
    const uint32_t n_docs = r->n_logs / replicas;
    if (n_docs) {
        hipLaunchKernelGGL(ptx_count_converged_kernel, dim3((n_docs + 255) / 256), dim3(256), 0, ctx->stream, r->logs, n_docs, replicas, (unsigned long long*)count_device);
        PTX_HIP(ctx, hipGetLastError());
    }
    return PTX_OK;
}

ptx_status ptx_calib_stream(ptx_ctx* ctx, const ptx_dbatch* b, uint64_t* bytes_read) {
    if (!ctx || !b || !bytes_read) return PTX_ERR_INVALID_ARG;
    PTX_HIP(ctx, ptx_enter(ctx));
    unsigned long long* d = nullptr;
    PTX_HIP(ctx, ptx_dev_malloc((void**)&d, 8));
    hipError_t e = hipMemsetAsync(d, 0, 8, ctx->stream);
    const bool env = b->chg_off != nullptr;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ptx_calib_stream_kernel, dim3(256 * 32), dim3(256), 0, ctx->stream, b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a,
                           b->side_b, b->n_ops, b->chg_hdr, b->chg_env, env ? b->n_changes : 0, b->max_actors, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)ptx_dev_free(d);
    if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("calibration stream: ") + hipGetErrorString(e));
    *bytes_read = 32 * b->n_ops + (env ? b->n_changes * (4 + 2ull * PTX_ENV_STRIDE(b->max_actors)) : 0);
    return PTX_OK;
}

ptx_status ptx_sync(ptx_ctx* ctx) {
    if (!ctx) return PTX_ERR_INVALID_ARG;
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PTX_OK;
}

/* ---- RCCL, bound at run time ---- */
struct PtxRccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static PtxRccl g_rccl;
static ptx_status rccl_load(ptx_ctx* ctx, const char* path = nullptr) {
    if (g_rccl.handle) return path ? fail(ctx, PTX_ERR_INVALID_ARG, "ptx_comm_use_library: a collective library is already bound in this process") : PTX_OK;
    /* the process may already hold RCCL (e.g. torch.distributed): the soname resolves to that copy */
    void* h = path ? dlopen(path, RTLD_NOW | RTLD_LOCAL) : dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h && !path) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h && !path) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(ctx, PTX_ERR_HIP, std::string("RCCL is not available: ") + dlerror());
    PtxRccl r;
    r.handle = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GetErrorString) return fail(ctx, PTX_ERR_HIP, "librccl lacks an expected symbol");
    g_rccl = r;
    return PTX_OK;
}
#define PTX_NCCL(ctx, call)                                                                          \
    do {                                                                                             \
        ncclResult_t _r = (call);                                                                    \
        if (_r != ncclSuccess) return fail(ctx, PTX_ERR_HIP, std::string(#call) + ": " + g_rccl.GetErrorString(_r)); \
    } while (0)

struct ptx_comm {
    ncclComm_t comm = nullptr;
    uint32_t rank = 0, n_ranks = 1;
    /* scratch of the unequal-block path */
    uint64_t *padded = nullptr, *mine = nullptr, *d_first = nullptr;
    uint32_t* d_counts = nullptr;
    uint32_t width = 0;
    std::vector<uint32_t> counts_up; /* the counts d_first / d_counts were last uploaded for: a steady loop (the same shard sizes step after
                                        step) uploads them once and has no host synchronisation inside the step */
    std::vector<uint64_t> first_up;
};

ptx_status ptx_comm_use_library(ptx_ctx* ctx, const char* path) {
    if (!ctx || !path || !*path) return PTX_ERR_INVALID_ARG;
    return rccl_load(ctx, path);
}

ptx_status ptx_comm_unique_id(ptx_ctx* ctx, uint8_t id[PTX_COMM_ID_BYTES]) {
    if (!ctx || !id) return PTX_ERR_INVALID_ARG;
    static_assert(sizeof(ncclUniqueId) == PTX_COMM_ID_BYTES, "ncclUniqueId size");
    ptx_status st = rccl_load(ctx);
    if (st) return st;
    ncclUniqueId u;
    PTX_NCCL(ctx, g_rccl.GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return PTX_OK;
}

ptx_status ptx_comm_init(ptx_ctx* ctx, const uint8_t id[PTX_COMM_ID_BYTES], uint32_t rank, uint32_t n_ranks, ptx_comm** out) {
    if (!ctx || !id || !out || n_ranks == 0 || rank >= n_ranks) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    ptx_status st = rccl_load(ctx);
    if (st) return st;
    PTX_HIP(ctx, ptx_enter(ctx));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ptx_comm* c = new ptx_comm();
    c->rank = rank;
    c->n_ranks = n_ranks;
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, (int)n_ranks, u, (int)rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(ctx, PTX_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
    }
    *out = c;
    return PTX_OK;
}

void ptx_comm_destroy(ptx_ctx* ctx, ptx_comm* c) {
    if (!c) return;
    if (ctx) {
        (void)ptx_enter(ctx);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    (void)ptx_dev_free(c->padded);
    (void)ptx_dev_free(c->mine);
    (void)ptx_dev_free(c->d_first);
    (void)ptx_dev_free(c->d_counts);
    delete c;
}

uint32_t ptx_comm_n_ranks(const ptx_comm* c) { return c ? c->n_ranks : 0u; }
uint32_t ptx_comm_rank(const ptx_comm* c) { return c ? c->rank : 0u; }

ptx_status ptx_allgather_digests(ptx_ctx* ctx, ptx_comm* c, const ptx_dresult* r, const uint32_t* counts, uint64_t* out_device) {
    if (!ctx || !c || !r || !counts || !out_device) return PTX_ERR_INVALID_ARG;
    if (counts[c->rank] != r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_allgather_digests: counts[rank] must be the logs of this rank's result");
    PTX_HIP(ctx, ptx_enter(ctx));
    uint32_t width = 0;
    bool equal = true;
    for (uint32_t k = 0; k < c->n_ranks; ++k) {
        width = std::max(width, counts[k]);
        equal = equal && counts[k] == counts[0];
    }
    if (width == 0) return PTX_OK;
    if (equal && !(ctx->flags & PTX_FLAG_PAD_GATHER)) {
        /* the digests go out packed from a staging block of this rank's slice of the output itself */
        uint64_t* mine = out_device + (uint64_t)c->rank * width * 2;
        hipLaunchKernelGGL(ptx_pack_digests_kernel, dim3((width + 255) / 256), dim3(256), 0, ctx->stream, r->logs, 0u, width, mine);
        PTX_HIP(ctx, hipGetLastError());
        PTX_NCCL(ctx, g_rccl.AllGather(mine, out_device, (size_t)width * 2, ncclUint64, c->comm, ctx->stream));
        return PTX_OK;
    }
    if (c->width < width) { /* (re)size the scratch of the padded path */
        (void)ptx_dev_free(c->padded);
        (void)ptx_dev_free(c->mine);
        c->padded = c->mine = nullptr;
        c->width = 0;
        PTX_HIP(ctx, dalloc(&c->padded, (uint64_t)c->n_ranks * width * 2));
        PTX_HIP(ctx, dalloc(&c->mine, (uint64_t)width * 2));
        if (!c->d_first) PTX_HIP(ctx, dalloc(&c->d_first, (uint64_t)c->n_ranks));
        if (!c->d_counts) PTX_HIP(ctx, dalloc(&c->d_counts, (uint64_t)c->n_ranks));
        c->width = width;
    }
    if (c->counts_up.size() != c->n_ranks || memcmp(c->counts_up.data(), counts, (size_t)c->n_ranks * 4) != 0) {
        /* new shard sizes (the first call, normally): block starts and counts go to the device once; the host copies live in the communicator */
        if (!c->counts_up.empty()) PTX_HIP(ctx, hipStreamSynchronize(ctx->stream)); /* an earlier upload may still be reading them */
        c->counts_up.assign(counts, counts + c->n_ranks);
        c->first_up.assign(c->n_ranks, 0);
        for (uint32_t k = 1; k < c->n_ranks; ++k) c->first_up[k] = c->first_up[k - 1] + counts[k - 1];
        PTX_HIP(ctx, hipMemcpyAsync(c->d_first, c->first_up.data(), (size_t)c->n_ranks * 8, hipMemcpyHostToDevice, ctx->stream));
        PTX_HIP(ctx, hipMemcpyAsync(c->d_counts, c->counts_up.data(), (size_t)c->n_ranks * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    PTX_HIP(ctx, hipMemsetAsync(c->mine, 0, (size_t)c->width * 16, ctx->stream));
    if (r->n_logs) {
        hipLaunchKernelGGL(ptx_pack_digests_kernel, dim3((r->n_logs + 255) / 256), dim3(256), 0, ctx->stream, r->logs, 0u, r->n_logs, c->mine);
        PTX_HIP(ctx, hipGetLastError());
    }
    PTX_NCCL(ctx, g_rccl.AllGather(c->mine, c->padded, (size_t)c->width * 2, ncclUint64, c->comm, ctx->stream));
    hipLaunchKernelGGL(ptx_compact_digests_kernel, dim3(std::min<uint32_t>((width * 2 + 255) / 256, 1024), c->n_ranks), dim3(256), 0, ctx->stream, c->padded, c->d_first,
                       c->d_counts, c->width, out_device);
    PTX_HIP(ctx, hipGetLastError());
    return PTX_OK;
}

ptx_status ptx_count_converged_digests(ptx_ctx* ctx, const uint64_t* digests_device, uint64_t n_logs, uint32_t replicas, uint64_t* count_device) {
    if (!ctx || !count_device || replicas == 0 || (!digests_device && n_logs)) return PTX_ERR_INVALID_ARG;
    if (n_logs % replicas) return fail(ctx, PTX_ERR_INVALID_ARG, "n_logs is not a multiple of replicas");
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, hipMemsetAsync(count_device, 0, 8, ctx->stream));
    const uint64_t n_docs = n_logs / replicas;
    if (n_docs) {
        hipLaunchKernelGGL(ptx_count_converged_digests_kernel, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, ctx->stream, digests_device, n_docs, replicas,
                           (unsigned long long*)count_device);
        PTX_HIP(ctx, hipGetLastError());
    }
    return PTX_OK;
}

ptx_status ptx_device_alloc(ptx_ctx* ctx, uint64_t bytes, void** out_device) {
    if (!ctx || !out_device) return PTX_ERR_INVALID_ARG;
    *out_device = nullptr;
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, ptx_dev_malloc(out_device, std::max<uint64_t>(bytes, 1)));
    return PTX_OK;
}
void ptx_device_free(ptx_ctx* ctx, void* device) {
    if (ctx) (void)ptx_enter(ctx);
    (void)ptx_dev_free(device);
}
ptx_status ptx_device_read(ptx_ctx* ctx, const void* device, void* host, uint64_t bytes) {
    if (!ctx || (bytes && (!device || !host))) return PTX_ERR_INVALID_ARG;
    PTX_HIP(ctx, ptx_enter(ctx));
    if (bytes) PTX_HIP(ctx, hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PTX_OK;
}

/* What a ptx_result owns (ABI 7: COMPACT rows).  The arrays a log's few rows go to are pinned host memory (the device writes them by DMA, nothing is
 * zero-filled, nothing is copied again); elem_rank — one entry per op row, hundreds of MB for a large batch, wanted by few callers — is plain memory. */
struct ptx_host_result {
    void* pinned[2] = {nullptr, nullptr}; /* [0] logs + the three offset arrays, [1] values + spans + cintervals */
    void* heap = nullptr;                 /* a SMALL range: one plain block for all of them, copied out of the context's pinned staging block */
    uint32_t* rank = nullptr;
    ~ptx_host_result() {
        for (void* p : pinned)
            if (p) (void)hipHostFree(p);
        free(heap);
        free(rank);
    }
};

void ptx_result_free(ptx_result* res) {
    if (!res) return;
    delete (ptx_host_result*)res->owner;
    memset(res, 0, sizeof(*res));
}

#define PTX_SMALL_DOWNLOAD_ROWS 65536ull /* ranges of up to this many op rows (a replica of an editor session): dense arrays sized by the rows, one allocation, one wait */
ptx_status ptx_result_download_range(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, uint32_t first_log, uint32_t n_logs, ptx_result* out) {
    if (!ctx || !b || !r || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if ((uint64_t)first_log + n_logs > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "log range exceeds the result");
    PTX_HIP(ctx, ptx_enter(ctx));
    uint64_t lo[2] = {0, 0};
    if (r->n_logs) {
        PTX_HIP(ctx, hipMemcpyAsync(&lo[0], b->log_off + first_log, 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_HIP(ctx, hipMemcpyAsync(&lo[1], b->log_off + first_log + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (lo[1] < lo[0] || lo[1] > r->n_rows) return fail(ctx, PTX_ERR_INVALID_ARG, "log_off is not monotonic");
    const uint64_t r0 = lo[0], nr = lo[1] - lo[0];
    ptx_host_result* h = new ptx_host_result();
    const uint64_t no = (uint64_t)n_logs + 1;
    const bool small = nr <= PTX_SMALL_DOWNLOAD_ROWS;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0: the per-log result rows and the offsets of the logs in the dense arrays (three exclusive prefix sums of their row counts, made on the device) */
    const uint64_t logs_bytes = a16((uint64_t)n_logs * sizeof(ptx_log_result)), off_bytes = a16(3 * no * 8);
    /* block 1: the dense rows.  A small range takes its row capacity as their size (known now: everything goes out in one batch of copies and one wait); a large
     * one waits for the totals first and allocates exactly those */
    uint64_t cv = nr, cs = nr, cc = nr;
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *dblk = nullptr, *dblk1 = nullptr;
    hipError_t e = hipSuccess;
    const uint64_t h0_bytes = logs_bytes + off_bytes + (small ? a16(cv * 4) + a16(cs * sizeof(ptx_span)) + a16(cc * sizeof(ptx_cinterval)) : 0) + 16;
    const uint64_t d0_bytes = off_bytes + (small ? a16(cv * 4) + a16(cs * sizeof(ptx_span)) + a16(cc * sizeof(ptx_cinterval)) : 0) + 16;
    if (small) { /* the context's own staging blocks (grown on demand, kept): no allocation, no hipFree — a device-wide wait — per read */
        if (ctx->stage_h_cap < h0_bytes) {
            if (ctx->stage_h) (void)hipHostFree(ctx->stage_h);
            ctx->stage_h = nullptr;
            ctx->stage_h_cap = 0;
            e = hipHostMalloc((void**)&ctx->stage_h, h0_bytes * 2, hipHostMallocDefault);
            if (e == hipSuccess) ctx->stage_h_cap = h0_bytes * 2;
        }
        if (e == hipSuccess && ctx->stage_d_cap < d0_bytes) {
            if (ctx->stage_d) (void)ptx_dev_free(ctx->stage_d);
            ctx->stage_d = nullptr;
            ctx->stage_d_cap = 0;
            e = ptx_dev_malloc((void**)&ctx->stage_d, d0_bytes * 2);
            if (e == hipSuccess) ctx->stage_d_cap = d0_bytes * 2;
        }
        hp0 = ctx->stage_h;
        dblk = ctx->stage_d;
    } else {
        e = hipHostMalloc((void**)&hp0, h0_bytes, hipHostMallocDefault);
        h->pinned[0] = hp0;
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&dblk, d0_bytes);
    }
    uint64_t* offs = (uint64_t*)(hp0 + logs_bytes);
    uint64_t* d_off = (uint64_t*)dblk;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ptx_result_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, r->logs, first_log, n_logs, d_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(offs, d_off, 3 * no * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && n_logs) e = hipMemcpyAsync(hp0, r->logs + first_log, (size_t)n_logs * sizeof(ptx_log_result), hipMemcpyDeviceToHost, ctx->stream);
    uint8_t* dense_h = nullptr;
    uint8_t* dense_d = nullptr;
    if (small) {
        dense_h = hp0 + logs_bytes + off_bytes;
        dense_d = dblk + off_bytes;
    } else {
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) {
            cv = offs[n_logs];
            cs = offs[no + n_logs];
            cc = offs[2 * no + n_logs];
            if (cv > nr || cs > nr || cc > nr) e = hipErrorInvalidValue; /* (a log never produces more rows than it has ops) */
        }
        const uint64_t dense_bytes = a16(cv * 4) + a16(cs * sizeof(ptx_span)) + a16(cc * sizeof(ptx_cinterval)) + 16;
        if (e == hipSuccess) e = hipHostMalloc((void**)&hp1, dense_bytes, hipHostMallocDefault);
        h->pinned[1] = hp1;
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&dblk1, dense_bytes);
        dense_h = hp1;
        dense_d = dblk1;
    }
    uint32_t* hv = (uint32_t*)dense_h;
    ptx_span* hs = (ptx_span*)(dense_h + a16(cv * 4));
    ptx_cinterval* hc = (ptx_cinterval*)(dense_h + a16(cv * 4) + a16(cs * sizeof(ptx_span)));
    if (e == hipSuccess && n_logs) {
        uint32_t* dv = (uint32_t*)dense_d;
        ptx_span* ds = (ptx_span*)(dense_d + a16(cv * 4));
        ptx_cinterval* dc = (ptx_cinterval*)(dense_d + a16(cv * 4) + a16(cs * sizeof(ptx_span)));
        hipLaunchKernelGGL(ptx_result_compact_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, b->log_off, r->logs, first_log, n_logs, d_off, r->values, r->spans, r->cints, dv, ds, dc);
        e = hipGetLastError();
        /* (a small range copies its capacity: the totals are not known on the host yet, and a few hundred KB cost less than a second wait) */
        if (e == hipSuccess && cv) e = hipMemcpyAsync(hv, dv, cv * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && cs) e = hipMemcpyAsync(hs, ds, cs * sizeof(ptx_span), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && cc) e = hipMemcpyAsync(hc, dc, cc * sizeof(ptx_cinterval), hipMemcpyDeviceToHost, ctx->stream);
    }
    /* elem_rank (where the context produces it): one entry per op row of the range, as the merge wrote it */
    if (e == hipSuccess && r->rank) {
        h->rank = (uint32_t*)malloc(std::max<uint64_t>(nr, 1) * 4);
        if (!h->rank) e = hipErrorOutOfMemory;
        else if (nr) e = hipMemcpyAsync(h->rank, r->rank + r0, nr * 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    else (void)hipStreamSynchronize(ctx->stream);
    if (!small) {
        (void)ptx_dev_free(dblk);
        (void)ptx_dev_free(dblk1);
    } else if (e == hipSuccess) { /* out of the staging block into memory the result owns (the rows that exist: a few KB for a replica of an editor session) */
        const uint64_t tv = offs[n_logs], ts = offs[no + n_logs], tc = offs[2 * no + n_logs];
        if (tv > nr || ts > nr || tc > nr) e = hipErrorInvalidValue;
        else {
            const uint64_t own_bytes = logs_bytes + off_bytes + a16(tv * 4) + a16(ts * sizeof(ptx_span)) + a16(tc * sizeof(ptx_cinterval)) + 16;
            uint8_t* own = (uint8_t*)malloc(own_bytes);
            if (!own) e = hipErrorOutOfMemory;
            else {
                memcpy(own, hp0, logs_bytes + off_bytes);
                uint8_t* dv2 = own + logs_bytes + off_bytes;
                memcpy(dv2, hv, tv * 4);
                memcpy(dv2 + a16(tv * 4), hs, ts * sizeof(ptx_span));
                memcpy(dv2 + a16(tv * 4) + a16(ts * sizeof(ptx_span)), hc, tc * sizeof(ptx_cinterval));
                h->heap = own;
                hp0 = own;
                offs = (uint64_t*)(own + logs_bytes);
                hv = (uint32_t*)dv2;
                hs = (ptx_span*)(dv2 + a16(tv * 4));
                hc = (ptx_cinterval*)(dv2 + a16(tv * 4) + a16(ts * sizeof(ptx_span)));
            }
        }
    }
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("result download: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->n_rows = nr;
    out->logs = (const ptx_log_result*)hp0;
    out->value_off = offs;
    out->span_off = offs + no;
    out->cint_off = offs + 2 * no;
    out->values = hv;
    out->spans = hs;
    out->cintervals = hc;
    out->elem_rank = r->rank ? h->rank : nullptr;
    out->owner = h;
    return PTX_OK;
}

ptx_status ptx_result_download(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, ptx_result* out) {
    if (!r) return PTX_ERR_INVALID_ARG;
    return ptx_result_download_range(ctx, b, r, 0, r->n_logs, out);
}

/* ---- document text: the resident string table and the assembled text of a range of logs (text_core.h) ---- */
struct ptx_dstrings {
    uint16_t* units = nullptr; /* device: the code units of all strings back to back */
    uint64_t* off = nullptr;   /* device [n + 1] */
    uint32_t n = 0;
    uint64_t n_units = 0;
};

ptx_status ptx_strings_upload(ptx_ctx* ctx, const uint16_t* units, const uint64_t* off, uint32_t n_strings, ptx_dstrings** out) {
    if (!ctx || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_strings && !off) return fail(ctx, PTX_ERR_INVALID_ARG, "string table without offsets");
    const uint64_t zero = 0;
    if (!n_strings) off = &zero;
    if (off[0] != 0) return fail(ctx, PTX_ERR_INVALID_ARG, "string offsets do not start at 0");
    for (uint32_t i = 0; i < n_strings; ++i)
        if (off[i + 1] < off[i]) return fail(ctx, PTX_ERR_INVALID_ARG, "string offsets are not monotonic");
    const uint64_t nu = off[n_strings];
    if (nu && !units) return fail(ctx, PTX_ERR_INVALID_ARG, "string table without code units");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dstrings* s = new ptx_dstrings();
    s->n = n_strings;
    s->n_units = nu;
    hipError_t e = ptx_dev_malloc((void**)&s->units, std::max<uint64_t>(nu, 1) * 2);
    if (e == hipSuccess) e = ptx_dev_malloc((void**)&s->off, ((uint64_t)n_strings + 1) * 8);
    if (e == hipSuccess && nu) e = hipMemcpyAsync(s->units, units, nu * 2, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->off, off, ((uint64_t)n_strings + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); /* the caller's arrays are pageable and free to go once this returns */
    else (void)hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)ptx_dev_free(s->units);
        (void)ptx_dev_free(s->off);
        delete s;
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("string table upload: ") + hipGetErrorString(e));
    }
    *out = s;
    return PTX_OK;
}
void ptx_strings_free(ptx_ctx* ctx, ptx_dstrings* s) {
    if (!s) return;
    if (ctx) (void)ptx_enter(ctx);
    (void)ptx_dev_free(s->units);
    (void)ptx_dev_free(s->off);
    delete s;
}

void ptx_text_free(ptx_text* t) {
    if (!t) return;
    delete (ptx_host_result*)t->owner;
    memset(t, 0, sizeof(*t));
}

ptx_status ptx_result_text_range(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs, ptx_text* out) {
    if (!ctx || !b || !r || !s || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if ((uint64_t)first_log + n_logs > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "log range exceeds the result");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_result* h = new ptx_host_result();
    const uint64_t no = (uint64_t)n_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0: the statuses and the two offset rows (text_off, span_off) — device and pinned host alike */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), blk0 = st_bytes + a16(2 * no * 8);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, blk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess) e = ptx_dev_malloc((void**)&d0, blk0);
    uint64_t* offs = (uint64_t*)(hp0 + st_bytes);
    float ms_len = 0.f, ms_asm = 0.f;
    uint64_t tu = 0, ts = 0;
    PtxTextArgs A;
    memset(&A, 0, sizeof(A));
    if (e == hipSuccess) {
        A.log_off = b->log_off;
        A.logs = r->logs;
        A.values = r->values;
        A.spans = r->spans;
        A.units = s->units;
        A.str_off = s->off;
        A.n_strings = s->n;
        A.first_log = first_log;
        A.n_logs = n_logs;
        A.status = (uint32_t*)d0;
        A.off = (uint64_t*)(d0 + st_bytes);
    }
    if (e == hipSuccess && n_logs) {
        e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_text_length_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0, d0, blk0, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_len, ctx->ev0, ctx->ev1);
        if (e == hipSuccess) {
            tu = offs[n_logs];
            ts = offs[no + n_logs];
            if (ts > r->n_rows) e = hipErrorInvalidValue; /* (a log never produces more rows than it has ops) */
        }
    } else if (e == hipSuccess) {
        offs[0] = offs[1] = 0; /* an empty range: text_off = span_off = {0} */
    }
    /* block 1: the text and the spans' unit offsets */
    const uint64_t tx_bytes = a16(tu * 2), blk1 = tx_bytes + a16(ts * 4) + 16;
    if (e == hipSuccess) e = hipHostMalloc((void**)&hp1, blk1, hipHostMallocDefault);
    h->pinned[1] = hp1;
    if (e == hipSuccess && n_logs) {
        e = ptx_dev_malloc((void**)&d1, blk1);
        if (e == hipSuccess) {
            A.text = (uint16_t*)d1;
            A.span_unit = (uint32_t*)(d1 + tx_bytes);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_text_assemble_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess && tu) e = hipMemcpyAsync(hp1, d1, tu * 2, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && ts) e = hipMemcpyAsync(hp1 + tx_bytes, d1 + tx_bytes, ts * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_asm, ctx->ev0, ctx->ev1);
    }
    (void)ptx_dev_free(d0);
    (void)ptx_dev_free(d1);
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("document text: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->kernel_ms = ms_len + ms_asm;
    out->status = (const uint32_t*)hp0;
    out->text_off = offs;
    out->span_off = offs + no;
    out->text = (const uint16_t*)hp1;
    out->span_unit = (const uint32_t*)(hp1 + tx_bytes);
    out->owner = h;
    return PTX_OK;
}

/* ---- find in the assembled text (find_core.h): the text passes above into a pool block that is never downloaded, then count, scan, emit.  Three waits: the text's
 *      size, the number of listed hits, the hits (a count-only call, or one without a hit, has two) ---- */
void ptx_matches_free(ptx_matches* m) {
    if (!m) return;
    delete (ptx_host_result*)m->owner;
    memset(m, 0, sizeof(*m));
}

ptx_status ptx_result_find_text(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs, const uint16_t* pattern,
                                uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log, ptx_matches* out) {
    if (!ctx || !b || !r || !s || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (!pattern || n_pattern == 0) return fail(ctx, PTX_ERR_INVALID_ARG, "empty pattern");
    if (n_pattern > PTX_FIND_PATTERN_MAX) return fail(ctx, PTX_ERR_INVALID_ARG, "pattern longer than PTX_FIND_PATTERN_MAX code units");
    if (flags & ~PTX_FIND_ASCII_NOCASE) return fail(ctx, PTX_ERR_INVALID_ARG, "unknown find flag");
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if ((uint64_t)first_log + n_logs > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "log range exceeds the result");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_result* h = new ptx_host_result();
    const uint64_t no = (uint64_t)n_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status | n_matches | hit_off — what comes down — | the text passes' two offset rows | the pattern */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), down0 = 2 * st_bytes + a16(no * 8), off_at = down0, pat_at = off_at + a16(2 * no * 8), blk0 = pat_at + a16((uint64_t)n_pattern * 2);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr, *d2 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, blk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess) e = ptx_dev_malloc((void**)&d0, blk0);
    uint64_t* hit_off = (uint64_t*)(hp0 + 2 * st_bytes);
    uint64_t* totals = (uint64_t*)(hp0 + off_at); /* [0] code units, [1] spans of the range */
    float ms[3] = {0.f, 0.f, 0.f};
    uint64_t tu = 0, ts = 0, nhits = 0;
    PtxFindArgs A;
    memset(&A, 0, sizeof(A));
    if (e == hipSuccess) {
        A.T.log_off = b->log_off;
        A.T.logs = r->logs;
        A.T.values = r->values;
        A.T.spans = r->spans;
        A.T.units = s->units;
        A.T.str_off = s->off;
        A.T.n_strings = s->n;
        A.T.first_log = first_log;
        A.T.n_logs = n_logs;
        A.T.status = (uint32_t*)d0;
        A.T.off = (uint64_t*)(d0 + off_at);
        A.n_matches = (uint32_t*)(d0 + st_bytes);
        A.hit_off = (uint64_t*)(d0 + 2 * st_bytes);
        A.pattern = (const uint16_t*)(d0 + pat_at);
        A.n_pattern = n_pattern;
        A.flags = flags;
        A.cap = max_hits_per_log;
        memcpy(hp0 + pat_at, pattern, (size_t)n_pattern * 2); /* the caller's pattern is free to go */
        hit_off[0] = 0;                                       /* an empty range: hit_off = {0} */
    }
    if (e == hipSuccess && n_logs) {
        e = hipMemcpyAsync(d0 + pat_at, hp0 + pat_at, (size_t)n_pattern * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_text_length_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A.T);
            hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.T.off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&totals[0], A.T.off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&totals[1], A.T.off + no + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) {
            tu = totals[0];
            ts = totals[1];
            if (ts > r->n_rows) e = hipErrorInvalidValue; /* (a log never produces more rows than it has ops) */
        }
    }
    /* block 1, device only: the text and the spans' unit offsets (scratch: the assemble pass writes them, nobody reads them) */
    const uint64_t tx_bytes = a16(tu * 2), blk1 = tx_bytes + a16(ts * 4) + 16;
    if (e == hipSuccess && n_logs) {
        e = ptx_dev_malloc((void**)&d1, blk1);
        if (e == hipSuccess) {
            A.T.text = (uint16_t*)d1;
            A.T.span_unit = (uint32_t*)(d1 + tx_bytes);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_text_assemble_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A.T);
            hipLaunchKernelGGL(ptx_find_count_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)A.n_matches, max_hits_per_log, A.hit_off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0, d0, down0, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) nhits = hit_off[n_logs];
    }
    /* block 2, device and pinned host alike: hit_unit | hit_start | hit_end */
    const uint64_t col = a16(nhits * 4), blk2 = 3 * col + 16;
    if (e == hipSuccess) e = hipHostMalloc((void**)&hp1, blk2, hipHostMallocDefault);
    h->pinned[1] = hp1;
    if (e == hipSuccess && nhits) {
        e = ptx_dev_malloc((void**)&d2, blk2);
        if (e == hipSuccess) {
            A.hit_unit = (uint32_t*)d2;
            A.hit_start = (uint32_t*)(d2 + col);
            A.hit_end = (uint32_t*)(d2 + 2 * col);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_find_emit_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp1, d2, 3 * col, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[2], ctx->ev0, ctx->ev1);
    }
    (void)ptx_dev_free(d0);
    (void)ptx_dev_free(d1);
    (void)ptx_dev_free(d2);
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("find text: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->n_pattern = n_pattern;
    out->kernel_ms = ms[0] + ms[1] + ms[2];
    out->status = (const uint32_t*)hp0;
    out->n_matches = (const uint32_t*)(hp0 + st_bytes);
    out->hit_off = hit_off;
    out->hit_unit = (const uint32_t*)hp1;
    out->hit_start = (const uint32_t*)(hp1 + col);
    out->hit_end = (const uint32_t*)(hp1 + 2 * col);
    out->owner = h;
    return PTX_OK;
}

/* ---- text and span rows of element ranges (slice_core.h): the text passes into a pool block that is never downloaded, then plan, prefix, bounds, scan, copy and
 *      span emit.  Three waits: the sizes of the text and of the prefix block; the sizes of the output; the output (a call without slices has one) ---- */
void ptx_slices_free(ptx_slices* m) {
    if (!m) return;
    delete (ptx_host_result*)m->owner;
    memset(m, 0, sizeof(*m));
}

/* the copy and span passes of ptx_result_text_slices, ptx_view_text_slices and ptx_view_find_snippets over bounds that are on the device, and their download: a block,
 * device and pinned host alike, of text | sspans | sspan_unit.  The pinned block becomes h->pinned[slot]; the device block goes back to the pool before this returns */
static hipError_t slice_emit_passes(ptx_ctx* ctx, PtxSliceArgs& A, uint64_t out_units, uint64_t out_rows, ptx_host_result* h, int slot, uint64_t* ot_bytes, uint64_t* os_bytes, float* ms) {
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    *ot_bytes = a16(out_units * 2);
    *os_bytes = a16(out_rows * sizeof(ptx_span));
    const uint64_t blk = *ot_bytes + *os_bytes + a16(out_rows * 4) + 16;
    uint8_t *hp = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp, blk, hipHostMallocDefault);
    h->pinned[slot] = hp;
    if (e == hipSuccess && (out_units || out_rows)) {
        e = ptx_dev_malloc((void**)&d, blk);
        if (e == hipSuccess) {
            A.out_text = (uint16_t*)d;
            A.out_spans = (ptx_span*)(d + *ot_bytes);
            A.out_span_unit = (uint32_t*)(d + *ot_bytes + *os_bytes);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            if (out_units) hipLaunchKernelGGL(ptx_slice_copy_kernel, dim3((uint32_t)((out_units + PTX_SLICE_BLOCK - 1) / PTX_SLICE_BLOCK)), dim3(64), 0, ctx->stream, A);
            if (out_rows) hipLaunchKernelGGL(ptx_slice_span_kernel, dim3((uint32_t)((out_rows + 255) / 256)), dim3(256), 0, ctx->stream, A, out_rows);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess && out_units) e = hipMemcpyAsync(hp, d, out_units * 2, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out_rows) e = hipMemcpyAsync(hp + *ot_bytes, d + *ot_bytes, *os_bytes + out_rows * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(ms, ctx->ev0, ctx->ev1);
        (void)ptx_dev_free(d);
    }
    return e;
}

ptx_status ptx_result_text_slices(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs, const uint64_t* slice_off,
                                  const uint32_t* slice_start, const uint32_t* slice_end, ptx_slices* out) {
    if (!ctx || !b || !r || !s || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if ((uint64_t)first_log + n_logs > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "log range exceeds the result");
    if (n_logs && !slice_off) return fail(ctx, PTX_ERR_INVALID_ARG, "slice_off is NULL");
    if (n_logs && slice_off[0] != 0) return fail(ctx, PTX_ERR_INVALID_ARG, "slice_off[0] is not 0");
    for (uint32_t l = 0; l < n_logs; ++l)
        if (slice_off[l + 1] < slice_off[l]) return fail(ctx, PTX_ERR_INVALID_ARG, "slice_off decreases");
    const uint64_t ns64 = n_logs ? slice_off[n_logs] : 0;
    if (ns64 > 0xFFFFFFFFull) return fail(ctx, PTX_ERR_INVALID_ARG, "more than 2^32 - 1 slices");
    if (ns64 && (!slice_start || !slice_end)) return fail(ctx, PTX_ERR_INVALID_ARG, "slices present but slice_start or slice_end is NULL");
    const uint32_t ns = (uint32_t)ns64;
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_result* h = new ptx_host_result();
    const uint64_t no = (uint64_t)n_logs + 1, nso = ns64 + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status | elem_start | elem_end | unit_off, sspan_off — what comes down — | slice_off | slice_start | slice_end — what
     * goes up — ; the device's goes on with the text passes' two offset rows | the plan's two | slice_log | first_span | src_off; the host's with three totals */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), col = a16(ns64 * 4), es_at = st_bytes, ee_at = es_at + col, oo_at = ee_at + col, down0 = oo_at + a16(2 * nso * 8);
    const uint64_t so_at = down0, ss_at = so_at + a16(no * 8), se_at = ss_at + col, up_end = se_at + col;
    const uint64_t hblk0 = up_end + 32;
    const uint64_t off_at = up_end, po_at = off_at + a16(2 * no * 8), sl_at = po_at + a16(2 * no * 8), fs_at = sl_at + col, src_at = fs_at + col, dblk0 = src_at + a16(ns64 * 8);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, hblk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess) e = ptx_dev_malloc((void**)&d0, dblk0);
    uint64_t* out_off = (uint64_t*)(hp0 + oo_at);
    uint64_t* totals = (uint64_t*)(hp0 + up_end); /* [0] code units, [1] spans of the range, [2] words of the prefix block */
    float ms[3] = {0.f, 0.f, 0.f};
    uint64_t tu = 0, ts = 0, tp = 0, out_units = 0, out_rows = 0;
    PtxSliceArgs A;
    memset(&A, 0, sizeof(A));
    if (e == hipSuccess) {
        A.T.log_off = b->log_off;
        A.T.logs = r->logs;
        A.T.values = r->values;
        A.T.spans = r->spans;
        A.T.units = s->units;
        A.T.str_off = s->off;
        A.T.n_strings = s->n;
        A.T.first_log = first_log;
        A.T.n_logs = n_logs;
        A.T.status = (uint32_t*)d0;
        A.T.off = (uint64_t*)(d0 + off_at);
        A.slice_off = (const uint64_t*)(d0 + so_at);
        A.slice_start = (const uint32_t*)(d0 + ss_at);
        A.slice_end = (const uint32_t*)(d0 + se_at);
        A.n_slices = ns;
        A.pre_off = (uint64_t*)(d0 + po_at);
        A.elem_start = (uint32_t*)(d0 + es_at);
        A.elem_end = (uint32_t*)(d0 + ee_at);
        A.out_off = (uint64_t*)(d0 + oo_at);
        A.slice_log = (uint32_t*)(d0 + sl_at);
        A.first_span = (uint32_t*)(d0 + fs_at);
        A.src_off = (uint64_t*)(d0 + src_at);
        /* the caller's arrays are free to go */
        if (n_logs) memcpy(hp0 + so_at, slice_off, (size_t)no * 8);
        if (ns) {
            memcpy(hp0 + ss_at, slice_start, (size_t)ns * 4);
            memcpy(hp0 + se_at, slice_end, (size_t)ns * 4);
        }
        out_off[0] = out_off[nso] = 0; /* no slices: unit_off = sspan_off = {0} */
    }
    if (e == hipSuccess && n_logs) {
        e = hipMemcpyAsync(d0 + so_at, hp0 + so_at, up_end - so_at, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_text_length_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A.T);
            hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.T.off, n_logs);
            if (ns) {
                hipLaunchKernelGGL(ptx_slice_plan_kernel, dim3((n_logs + 255u) / 256u), dim3(256), 0, ctx->stream, A);
                hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.pre_off, n_logs);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0, d0, (size_t)n_logs * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&totals[0], A.T.off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&totals[1], A.T.off + no + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && ns) e = hipMemcpyAsync(&totals[2], A.pre_off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) {
            tu = totals[0];
            ts = totals[1];
            tp = ns ? totals[2] : 0;
            if (ts > r->n_rows || tp > r->n_rows + n_logs) e = hipErrorInvalidValue; /* (a log never produces more rows than it has ops) */
        }
    }
    /* block 1, device only: the text, the spans' unit offsets (the assemble pass writes them, nobody reads them) and the element prefixes */
    const uint64_t tx_bytes = a16(tu * 2), su_bytes = a16(ts * 4), blk1 = tx_bytes + su_bytes + a16(tp * 4) + 16;
    if (e == hipSuccess && ns) {
        e = ptx_dev_malloc((void**)&d1, blk1);
        if (e == hipSuccess) {
            A.T.text = (uint16_t*)d1;
            A.T.span_unit = (uint32_t*)(d1 + tx_bytes);
            A.pre = (uint32_t*)(d1 + tx_bytes + su_bytes);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_text_assemble_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A.T);
            hipLaunchKernelGGL(ptx_slice_prefix_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            hipLaunchKernelGGL(ptx_slice_bounds_kernel, dim3((uint32_t)((ns64 + 255) / 256)), dim3(256), 0, ctx->stream, A);
            hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.out_off, ns);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + es_at, d0 + es_at, down0 - es_at, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) {
            out_units = out_off[ns];
            out_rows = out_off[nso + ns];
        }
    }
    /* block 2, device and pinned host alike: text | sspans | sspan_unit */
    uint64_t ot_bytes = 0, os_bytes = 0;
    if (e == hipSuccess) e = slice_emit_passes(ctx, A, out_units, out_rows, h, 1, &ot_bytes, &os_bytes, &ms[2]);
    hp1 = (uint8_t*)h->pinned[1];
    (void)ptx_dev_free(d0);
    (void)ptx_dev_free(d1);
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("text slices: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->n_slices = ns;
    out->kernel_ms = ms[0] + ms[1] + ms[2];
    out->status = (const uint32_t*)hp0;
    out->elem_start = (const uint32_t*)(hp0 + es_at);
    out->elem_end = (const uint32_t*)(hp0 + ee_at);
    out->unit_off = out_off;
    out->sspan_off = out_off + nso;
    out->text = (const uint16_t*)hp1;
    out->sspans = (const ptx_span*)(hp1 + ot_bytes);
    out->sspan_unit = (const uint32_t*)(hp1 + ot_bytes + os_bytes);
    out->owner = h;
    return PTX_OK;
}

/* ---- a resident text view (view_core.h): the text passes and the element prefix of EVERY good log once, into blocks the view owns (plain hipMalloc: they are
 *      large and live long, the pool of small blocks is for a call's scratch); then queries that run the find and slice passes over them.  Creation has two
 *      waits: the sizes, the blocks.  A find has two (the number of listed hits, the hits), a slice call two (the sizes of the output, the output), a snippet
 *      call three: what it saves over find + slices is every text and prefix pass, and the hits' trip to the host and back ---- */
struct ptx_dview {
    const ptx_dresult* r = nullptr; /* its span rows are read by slice and snippet calls */
    uint32_t first_log = 0, n_logs = 0;
    uint64_t n_units = 0, n_spans = 0, n_pre = 0, bytes = 0;
    float kernel_ms = 0.f;
    uint8_t *d0 = nullptr, *d1 = nullptr; /* d0: status | text_off, span_off | pre_off (two rows) | log_off | the plan's slice_off;  d1: text | span_unit | pre */
    uint32_t* status = nullptr;
    uint64_t *off = nullptr, *pre_off = nullptr, *log_off = nullptr;
    uint16_t* text = nullptr;
    uint32_t *span_unit = nullptr, *pre = nullptr;
    std::vector<uint32_t> h_status; /* every query's result starts with it */
};

/* the text passes' arguments as a query sees them: the range is rebased to log 0 of the view's own log_off; no per-log rows, no values, no string table */
static void view_text_args(const ptx_dview* v, PtxTextArgs& T) {
    memset(&T, 0, sizeof(T));
    T.log_off = v->log_off;
    T.logs = nullptr; /* ptx_slice_visible then takes n_visible from the view's own prefix: the view and the bounds pass cannot disagree */
    T.spans = v->r ? v->r->spans : nullptr;
    T.first_log = 0;
    T.n_logs = v->n_logs;
    T.status = v->status;
    T.off = v->off;
    T.text = v->text;
    T.span_unit = v->span_unit;
}

void ptx_text_view_free(ptx_ctx* ctx, ptx_dview* v) {
    if (!v) return;
    if (ctx) (void)ptx_enter(ctx);
    (void)hipFree(v->d0);
    (void)hipFree(v->d1);
    delete v;
}

ptx_status ptx_text_view_create(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs, ptx_dview** out) {
    if (!ctx || !b || !r || !s || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if ((uint64_t)first_log + n_logs > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "log range exceeds the result");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dview* v = new ptx_dview();
    v->r = r;
    v->first_log = first_log;
    v->n_logs = n_logs;
    v->h_status.resize(n_logs);
    if (n_logs == 0) { /* the empty view holds nothing */
        *out = v;
        return PTX_OK;
    }
    const uint64_t no = (uint64_t)n_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), off_at = st_bytes, po_at = off_at + a16(2 * no * 8), lo_at = po_at + a16(2 * no * 8), so_at = lo_at + a16(no * 8),
                   blk0 = so_at + a16(no * 8);
    float ms[2] = {0.f, 0.f};
    uint64_t totals[3] = {0, 0, 0}; /* code units, spans, words of the prefix */
    PtxSliceArgs A;
    memset(&A, 0, sizeof(A));
    hipError_t e = hipMalloc((void**)&v->d0, blk0);
    if (e == hipSuccess) {
        v->status = (uint32_t*)v->d0;
        v->off = (uint64_t*)(v->d0 + off_at);
        v->pre_off = (uint64_t*)(v->d0 + po_at);
        v->log_off = (uint64_t*)(v->d0 + lo_at);
        A.T.log_off = b->log_off;
        A.T.logs = r->logs;
        A.T.values = r->values;
        A.T.spans = r->spans;
        A.T.units = s->units;
        A.T.str_off = s->off;
        A.T.n_strings = s->n;
        A.T.first_log = first_log;
        A.T.n_logs = n_logs;
        A.T.status = v->status;
        A.T.off = v->off;
        A.slice_off = (const uint64_t*)(v->d0 + so_at);
        A.n_slices = n_logs;
        A.pre_off = v->pre_off;
        e = hipMemcpyAsync(v->log_off, b->log_off + first_log, no * 8, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ptx_text_length_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A.T);
        hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.T.off, n_logs);
        hipLaunchKernelGGL(ptx_view_plan_kernel, dim3((n_logs + 255u) / 256u), dim3(256), 0, ctx->stream, A, (uint64_t*)(v->d0 + so_at));
        hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.pre_off, n_logs);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v->h_status.data(), v->status, (size_t)n_logs * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&totals[0], A.T.off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&totals[1], A.T.off + no + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&totals[2], A.pre_off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    else (void)hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
    if (e == hipSuccess && (totals[1] > r->n_rows || totals[2] > r->n_rows + n_logs)) e = hipErrorInvalidValue; /* (a log never produces more rows than it has ops) */
    const uint64_t tx_bytes = a16(totals[0] * 2), su_bytes = a16(totals[1] * 4), blk1 = tx_bytes + su_bytes + a16(totals[2] * 4) + 16;
    if (e == hipSuccess) e = hipMalloc((void**)&v->d1, blk1);
    if (e == hipSuccess) {
        A.T.text = v->text = (uint16_t*)v->d1;
        A.T.span_unit = v->span_unit = (uint32_t*)(v->d1 + tx_bytes);
        A.pre = v->pre = (uint32_t*)(v->d1 + tx_bytes + su_bytes);
        e = hipEventRecord(ctx->ev0, ctx->stream);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ptx_text_assemble_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A.T);
        hipLaunchKernelGGL(ptx_slice_prefix_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); /* the batch and the strings are free to go once this returns */
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
    }
    if (e != hipSuccess) {
        ptx_text_view_free(ctx, v);
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("text view: ") + hipGetErrorString(e));
    }
    v->n_units = totals[0];
    v->n_spans = totals[1];
    v->n_pre = totals[2];
    v->bytes = blk0 + blk1;
    v->kernel_ms = ms[0] + ms[1];
    *out = v;
    return PTX_OK;
}

ptx_status ptx_view_info(ptx_ctx* ctx, const ptx_dview* v, ptx_view_desc* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->n_logs = v->n_logs;
    out->first_log = v->first_log;
    out->n_units = v->n_units;
    out->n_prefix_words = v->n_pre;
    out->bytes = v->bytes;
    out->kernel_ms = v->kernel_ms;
    return PTX_OK;
}

/* what a ptx_snippets owns: the find's two pinned blocks and the snippets' one */
struct ptx_host_snippets {
    ptx_host_result find, cut;
};

void ptx_snippets_free(ptx_snippets* m) {
    if (!m) return;
    delete (ptx_host_snippets*)m->owner;
    memset(m, 0, sizeof(*m));
}

/* ptx_view_find_text (snip == false: `cut` is not used) and ptx_view_find_snippets; the arguments are checked */
static ptx_status view_find_impl(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log, bool snip, uint32_t before,
                                 uint32_t after, ptx_host_result* h, ptx_host_result* cut, ptx_snippets* out) {
    PTX_HIP(ctx, ptx_enter(ctx));
    const uint32_t n_logs = v->n_logs;
    const uint64_t no = (uint64_t)n_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status (the host's only: the view keeps the device's) | n_matches | hit_off — what comes down — | the pattern */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), down0 = 2 * st_bytes + a16(no * 8), pat_at = down0, blk0 = pat_at + a16((uint64_t)n_pattern * 2);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, blk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess) e = ptx_dev_malloc((void**)&d0, blk0);
    uint64_t* hit_off = (uint64_t*)(hp0 + 2 * st_bytes);
    float ms[3] = {0.f, 0.f, 0.f};
    uint64_t nhits = 0, out_units = 0, out_rows = 0, ot_bytes = 0, os_bytes = 0;
    bool too_many = false;
    PtxViewArgs V;
    memset(&V, 0, sizeof(V));
    if (e == hipSuccess) {
        view_text_args(v, V.F.T);
        V.F.n_matches = (uint32_t*)(d0 + st_bytes);
        V.F.hit_off = (uint64_t*)(d0 + 2 * st_bytes);
        V.F.pattern = (const uint16_t*)(d0 + pat_at);
        V.F.n_pattern = n_pattern;
        V.F.flags = flags;
        V.F.cap = max_hits_per_log;
        V.pre_off = v->pre_off;
        V.pre = v->pre;
        V.before = before;
        V.after = after;
        if (n_logs) memcpy(hp0, v->h_status.data(), (size_t)n_logs * 4);
        memcpy(hp0 + pat_at, pattern, (size_t)n_pattern * 2); /* the caller's pattern is free to go */
        hit_off[0] = 0;                                       /* an empty view: hit_off = {0} */
    }
    if (e == hipSuccess && n_logs) {
        e = hipMemcpyAsync(d0 + pat_at, hp0 + pat_at, (size_t)n_pattern * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_find_count_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, V.F);
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)V.F.n_matches, max_hits_per_log, V.F.hit_off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + st_bytes, d0 + st_bytes, down0 - st_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) nhits = hit_off[n_logs];
        if (e == hipSuccess && nhits > 0xFFFFFFFFull) too_many = true, e = hipErrorInvalidValue; /* a lane per listed hit, a slice per hit */
    }
    /* block 1, device and pinned host alike: hit_unit | hit_start | hit_end and, for snippets, | elem_start | elem_end | match_unit | unit_off, sspan_off — all of
     * it comes down in one copy, nothing goes up —; the device's goes on with win_start | win_end | slice_log | first_span | src_off */
    const uint64_t nso = nhits + 1, col = a16(nhits * 4), oo_at = (snip ? 6 : 3) * col, down1 = oo_at + (snip ? a16(2 * nso * 8) : 0), hblk1 = down1 + 16;
    const uint64_t ws_at = down1, sl_at = ws_at + 2 * col, src_at = sl_at + 2 * col, dblk1 = snip ? src_at + a16(nhits * 8) + 16 : hblk1;
    if (e == hipSuccess) e = hipHostMalloc((void**)&hp1, hblk1, hipHostMallocDefault);
    h->pinned[1] = hp1;
    uint64_t* out_off = (uint64_t*)(hp1 + oo_at);
    if (e == hipSuccess && snip) out_off[0] = out_off[nso] = 0; /* no hits: unit_off = sspan_off = {0} */
    PtxSliceArgs S;
    memset(&S, 0, sizeof(S));
    if (e == hipSuccess && nhits) {
        e = ptx_dev_malloc((void**)&d1, dblk1);
        if (e == hipSuccess) {
            V.n_hits = (uint32_t)nhits;
            V.F.hit_unit = (uint32_t*)d1;
            V.F.hit_start = (uint32_t*)(d1 + col);
            V.F.hit_end = (uint32_t*)(d1 + 2 * col);
            if (snip) {
                V.match_unit = (uint32_t*)(d1 + 5 * col);
                V.win_start = (uint32_t*)(d1 + ws_at);
                V.win_end = (uint32_t*)(d1 + ws_at + col);
                S.T = V.F.T;
                S.slice_off = V.F.hit_off; /* one slice per listed hit, in hit order */
                S.slice_start = V.win_start;
                S.slice_end = V.win_end;
                S.n_slices = (uint32_t)nhits;
                S.pre_off = v->pre_off;
                S.pre = v->pre;
                S.elem_start = (uint32_t*)(d1 + 3 * col);
                S.elem_end = (uint32_t*)(d1 + 4 * col);
                S.out_off = (uint64_t*)(d1 + oo_at);
                S.slice_log = (uint32_t*)(d1 + sl_at);
                S.first_span = (uint32_t*)(d1 + sl_at + col);
                S.src_off = (uint64_t*)(d1 + src_at);
            }
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            const uint32_t grid = (uint32_t)((nhits + 255) / 256);
            hipLaunchKernelGGL(ptx_view_positions_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, V.F);
            hipLaunchKernelGGL(ptx_view_locate_kernel, dim3(grid), dim3(256), 0, ctx->stream, V);
            if (snip) {
                hipLaunchKernelGGL(ptx_view_windows_kernel, dim3(grid), dim3(256), 0, ctx->stream, V);
                hipLaunchKernelGGL(ptx_slice_bounds_kernel, dim3(grid), dim3(256), 0, ctx->stream, S);
                hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, S.out_off, (uint32_t)nhits);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp1, d1, snip ? oo_at + 2 * nso * 8 : 3 * col, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
        if (e == hipSuccess && snip) {
            out_units = out_off[nhits];
            out_rows = out_off[nso + nhits];
        }
    }
    if (e == hipSuccess && snip) e = slice_emit_passes(ctx, S, out_units, out_rows, cut, 0, &ot_bytes, &os_bytes, &ms[2]);
    (void)ptx_dev_free(d0);
    (void)ptx_dev_free(d1);
    if (e != hipSuccess) {
        if (too_many) return fail(ctx, PTX_ERR_CAPACITY, "more than 2^32 - 1 listed hits: lower max_hits_per_log or the range");
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("view find: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->n_pattern = n_pattern;
    out->kernel_ms = ms[0] + ms[1] + ms[2];
    out->n_slices = snip ? (uint32_t)nhits : 0u;
    out->status = (const uint32_t*)hp0;
    out->n_matches = (const uint32_t*)(hp0 + st_bytes);
    out->hit_off = hit_off;
    out->hit_unit = (const uint32_t*)hp1;
    out->hit_start = (const uint32_t*)(hp1 + col);
    out->hit_end = (const uint32_t*)(hp1 + 2 * col);
    if (snip) {
        const uint8_t* hp2 = (const uint8_t*)cut->pinned[0];
        out->elem_start = (const uint32_t*)(hp1 + 3 * col);
        out->elem_end = (const uint32_t*)(hp1 + 4 * col);
        out->match_unit = (const uint32_t*)(hp1 + 5 * col);
        out->unit_off = out_off;
        out->sspan_off = out_off + nso;
        out->text = (const uint16_t*)hp2;
        out->sspans = (const ptx_span*)(hp2 + ot_bytes);
        out->sspan_unit = (const uint32_t*)(hp2 + ot_bytes + os_bytes);
    }
    return PTX_OK;
}

static ptx_status view_find_check(ptx_ctx* ctx, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags) {
    if (!pattern || n_pattern == 0) return fail(ctx, PTX_ERR_INVALID_ARG, "empty pattern");
    if (n_pattern > PTX_FIND_PATTERN_MAX) return fail(ctx, PTX_ERR_INVALID_ARG, "pattern longer than PTX_FIND_PATTERN_MAX code units");
    if (flags & ~PTX_FIND_ASCII_NOCASE) return fail(ctx, PTX_ERR_INVALID_ARG, "unknown find flag");
    return PTX_OK;
}

ptx_status ptx_view_find_text(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log, ptx_matches* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_status st = view_find_check(ctx, pattern, n_pattern, flags);
    if (st != PTX_OK) return st;
    ptx_host_result* h = new ptx_host_result();
    ptx_snippets m;
    memset(&m, 0, sizeof(m));
    st = view_find_impl(ctx, v, pattern, n_pattern, flags, max_hits_per_log, false, 0u, 0u, h, nullptr, &m);
    if (st != PTX_OK) {
        delete h;
        return st;
    }
    out->n_logs = m.n_logs;
    out->n_pattern = m.n_pattern;
    out->kernel_ms = m.kernel_ms;
    out->status = m.status;
    out->n_matches = m.n_matches;
    out->hit_off = m.hit_off;
    out->hit_unit = m.hit_unit;
    out->hit_start = m.hit_start;
    out->hit_end = m.hit_end;
    out->owner = h;
    return PTX_OK;
}

ptx_status ptx_view_find_snippets(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log, uint32_t before, uint32_t after,
                                  ptx_snippets* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_status st = view_find_check(ctx, pattern, n_pattern, flags);
    if (st != PTX_OK) return st;
    ptx_host_snippets* h = new ptx_host_snippets();
    st = view_find_impl(ctx, v, pattern, n_pattern, flags, max_hits_per_log, true, before, after, &h->find, &h->cut, out);
    if (st != PTX_OK) {
        delete h;
        memset(out, 0, sizeof(*out));
        return st;
    }
    out->owner = h;
    return PTX_OK;
}

/* ---- find and replace on a view (replace_core.h): count -> offsets -> positions -> locate -> select -> the two scans -> the sizes come down -> emit -> one
 *      download.  Three waits: the number of hits, the number of Changes and ops, the plan.  The hits themselves never leave the device ---- */
void ptx_replace_plan_free(ptx_replace_plan* m) {
    if (!m) return;
    delete (ptx_host_result*)m->owner;
    memset(m, 0, sizeof(*m));
}

/* the arguments are checked; h->pinned[0]: status | n_matches | n_chosen | n_replaced | hit_off (scratch) | chg_off,  h->pinned[1]: op_off | index | count | payload |
 * action | mark_type | values */
static ptx_status view_replace_impl(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, const uint32_t* replacement, uint32_t n_replacement,
                                    uint32_t n_batch_logs, ptx_host_result* h, ptx_replace_plan* out, ptx_dinput_ops* keep = nullptr, const uint32_t* actor = nullptr,
                                    uint32_t max_actors = 0) {
    /* `keep` (ptx_view_replace_plan_device): the same passes; the op columns, chg_off and op_off are not brought down — their blocks are handed to `keep`, with
     * a third block that holds a zero (the op_off of a plan without ops), `actor` and the replacement's value ids */
    PTX_HIP(ctx, ptx_enter(ctx));
    const uint32_t n_logs = v->n_logs;
    const uint64_t no = (uint64_t)n_logs + 1, nbo = (uint64_t)n_batch_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status | n_matches | n_chosen | n_replaced | hit_off | chg_off — what comes down — | n_ops | makes | op_log_off | the pattern */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), ho_at = 4 * st_bytes, co_at = ho_at + a16(no * 8), down0 = co_at + a16(nbo * 8);
    const uint64_t no_at = down0, mk_at = no_at + st_bytes, ol_at = mk_at + a16((uint64_t)n_batch_logs * 4), pat_at = ol_at + a16(no * 8), blk0 = pat_at + a16((uint64_t)n_pattern * 2);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr, *d2 = nullptr, *d3 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, blk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess) e = ptx_dev_malloc((void**)&d0, blk0);
    const uint64_t act_at = 16, rv_at = act_at + a16((uint64_t)n_batch_logs * 4), blk3 = rv_at + a16((uint64_t)n_replacement * 4) + 16;
    if (keep) { /* the third block goes up first, through the context's pinned staging; chg_off of a view without hits is zeroed where the scan would write it */
        if (e == hipSuccess && ctx->up_h_cap < blk3) {
            if (ctx->up_h) (void)hipHostFree(ctx->up_h);
            ctx->up_h = nullptr;
            ctx->up_h_cap = 0;
            e = hipHostMalloc((void**)&ctx->up_h, 2 * blk3, hipHostMallocDefault);
            if (e == hipSuccess) ctx->up_h_cap = 2 * blk3;
        }
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d3, blk3);
        if (e == hipSuccess) {
            memset(ctx->up_h, 0, 16);
            if (n_batch_logs) memcpy(ctx->up_h + act_at, actor, (size_t)n_batch_logs * 4);
            if (n_replacement) memcpy(ctx->up_h + rv_at, replacement, (size_t)n_replacement * 4);
            e = hipMemcpyAsync(d3, ctx->up_h, blk3 - 16, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e == hipSuccess) e = hipMemsetAsync(d0 + co_at, 0, nbo * 8, ctx->stream);
    }
    float ms[3] = {0.f, 0.f, 0.f};
    uint64_t nhits = 0, sizes[2] = {0, 0}; /* Changes, InputOperations */
    bool too_many = false;
    PtxReplaceArgs R;
    memset(&R, 0, sizeof(R));
    if (e == hipSuccess) {
        memset(hp0, 0, blk0); /* an empty view, a view without hits: the all-zero plan */
        view_text_args(v, R.V.F.T);
        R.V.F.n_matches = (uint32_t*)(d0 + st_bytes);
        R.V.F.hit_off = (uint64_t*)(d0 + ho_at);
        R.V.F.pattern = (const uint16_t*)(d0 + pat_at);
        R.V.F.n_pattern = n_pattern;
        R.V.F.flags = flags;
        R.V.F.cap = 0xFFFFFFFFu;
        R.V.pre_off = v->pre_off;
        R.V.pre = v->pre;
        R.n_replacement = n_replacement;
        R.first_log = v->first_log;
        R.n_batch_logs = n_batch_logs;
        R.status = (uint32_t*)d0;
        R.n_chosen = (uint32_t*)(d0 + 2 * st_bytes);
        R.n_replaced = (uint32_t*)(d0 + 3 * st_bytes);
        R.chg_off = (uint64_t*)(d0 + co_at);
        R.n_ops = (uint32_t*)(d0 + no_at);
        R.makes = (uint32_t*)(d0 + mk_at);
        R.op_log_off = (uint64_t*)(d0 + ol_at);
        if (n_logs) memcpy(hp0, v->h_status.data(), (size_t)n_logs * 4);
        memcpy(hp0 + pat_at, pattern, (size_t)n_pattern * 2); /* the caller's pattern is free to go */
    }
    const uint64_t* hit_off = (const uint64_t*)(hp0 + ho_at);
    if (e == hipSuccess && n_logs) {
        e = hipMemcpyAsync(d0 + pat_at, hp0 + pat_at, (size_t)n_pattern * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_find_count_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, R.V.F);
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)R.V.F.n_matches, 0xFFFFFFFFu, R.V.F.hit_off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + st_bytes, d0 + st_bytes, st_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + ho_at, d0 + ho_at, no * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) nhits = hit_off[n_logs];
        if (e == hipSuccess && nhits > 0xFFFFFFFFull) too_many = true, e = hipErrorInvalidValue; /* a lane per hit */
    }
    /* block 1, the device's only: hit_unit | hit_start | hit_end | sel */
    const uint64_t col = a16(nhits * 4);
    if (e == hipSuccess && nhits) {
        e = ptx_dev_malloc((void**)&d1, 4 * col + 16);
        if (e == hipSuccess) {
            R.V.n_hits = (uint32_t)nhits;
            R.V.F.hit_unit = (uint32_t*)d1;
            R.V.F.hit_start = (uint32_t*)(d1 + col);
            R.V.F.hit_end = (uint32_t*)(d1 + 2 * col);
            R.sel = (uint32_t*)(d1 + 3 * col);
            e = hipMemsetAsync(R.makes, 0, (size_t)n_batch_logs * 4, ctx->stream); /* the logs outside the view's range make no Change */
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_view_positions_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, R.V.F);
            hipLaunchKernelGGL(ptx_view_locate_kernel, dim3((uint32_t)((nhits + 255) / 256)), dim3(256), 0, ctx->stream, R.V);
            hipLaunchKernelGGL(ptx_replace_select_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, R);
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)R.makes, 0xFFFFFFFFu, R.chg_off, n_batch_logs);
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)R.n_ops, 0xFFFFFFFFu, R.op_log_off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&sizes[0], R.chg_off + n_batch_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&sizes[1], R.op_log_off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
        if (e == hipSuccess && (sizes[0] > n_logs || sizes[1] > 2 * nhits)) e = hipErrorInvalidValue; /* (a Change per log, two ops per hit at the most) */
    }
    /* block 2, device and pinned host alike: op_off | index | count | payload | action | mark_type; the host's goes on with the value ids */
    const uint64_t nc = sizes[0], ni = sizes[1], oo_bytes = a16((nc + 1) * 8), c4 = a16(ni * 4), c1 = a16(ni), val_at = oo_bytes + 3 * c4 + 2 * c1,
                   blk2 = val_at + a16((uint64_t)n_replacement * 4) + 16;
    if (e == hipSuccess && !keep) e = hipHostMalloc((void**)&hp1, blk2, hipHostMallocDefault);
    h->pinned[1] = hp1;
    if (e == hipSuccess && !keep) {
        memset(hp1, 0, oo_bytes); /* no Change: op_off = {0} */
        if (n_replacement) memcpy(hp1 + val_at, replacement, (size_t)n_replacement * 4); /* the caller's ids are free to go */
    }
    if (e == hipSuccess && ni) {
        e = ptx_dev_malloc((void**)&d2, val_at + 16);
        if (e == hipSuccess) {
            R.op_off = (uint64_t*)d2;
            R.index = (uint32_t*)(d2 + oo_bytes);
            R.count = (uint32_t*)(d2 + oo_bytes + c4);
            R.payload = (uint32_t*)(d2 + oo_bytes + 2 * c4);
            R.action = d2 + oo_bytes + 3 * c4;
            R.mark_type = d2 + oo_bytes + 3 * c4 + c1;
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_replace_emit_kernel, dim3((uint32_t)((nhits + 255) / 256)), dim3(256), 0, ctx->stream, R);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess && !keep) e = hipMemcpyAsync(hp1, d2, val_at, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess && nhits) { /* the plan's status and counts, and chg_off: with the ops, one wait */
        e = hipMemcpyAsync(hp0, d0, st_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + 2 * st_bytes, d0 + 2 * st_bytes, 2 * st_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && !keep) e = hipMemcpyAsync(hp0 + co_at, d0 + co_at, nbo * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && ni) e = hipEventElapsedTime(&ms[2], ctx->ev0, ctx->ev1);
    } else if (keep) { /* (the staging block is free again when the call returns) */
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = e2;
    }
    if (keep && e == hipSuccess) { /* the blocks are handed over, not copied and freed */
        keep->n_logs = n_batch_logs;
        keep->max_actors = max_actors;
        keep->n_changes = nc;
        keep->n_input_ops = ni;
        keep->n_values = n_replacement;
        keep->owns = true;
        keep->blocks[0] = d0;
        keep->blocks[1] = d2;
        keep->blocks[2] = d3;
        keep->chg_off = (uint64_t*)(d0 + co_at);
        keep->op_off = ni ? (uint64_t*)d2 : (uint64_t*)d3;
        keep->index = ni ? R.index : nullptr;
        keep->count = ni ? R.count : nullptr;
        keep->payload = ni ? R.payload : nullptr;
        keep->action = ni ? R.action : nullptr;
        keep->mark_type = ni ? R.mark_type : nullptr;
        keep->actor = (uint32_t*)(d3 + act_at);
        keep->values = (uint32_t*)(d3 + rv_at);
        d0 = d2 = d3 = nullptr;
    }
    (void)ptx_dev_free(d0);
    (void)ptx_dev_free(d1);
    (void)ptx_dev_free(d2);
    (void)ptx_dev_free(d3);
    if (e != hipSuccess) {
        if (too_many) return fail(ctx, PTX_ERR_CAPACITY, "more than 2^32 - 1 matches in the view: plan a smaller range");
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("view replace plan: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->n_pattern = n_pattern;
    out->kernel_ms = ms[0] + ms[1] + ms[2];
    out->n_replacement = n_replacement;
    out->status = (const uint32_t*)hp0;
    out->n_matches = (const uint32_t*)(hp0 + st_bytes);
    out->n_chosen = (const uint32_t*)(hp0 + 2 * st_bytes);
    out->n_replaced = (const uint32_t*)(hp0 + 3 * st_bytes);
    out->ops.n_logs = n_batch_logs;
    out->ops.n_values = n_replacement;
    if (keep) { /* the ops stay on the device: no pointer of out->ops is set */
        out->ops.max_actors = max_actors;
        return PTX_OK;
    }
    out->ops.max_actors = 0;
    out->ops.chg_off = (const uint64_t*)(hp0 + co_at);
    out->ops.op_off = (const uint64_t*)hp1;
    out->ops.index = (const uint32_t*)(hp1 + oo_bytes);
    out->ops.count = (const uint32_t*)(hp1 + oo_bytes + c4);
    out->ops.payload = (const uint32_t*)(hp1 + oo_bytes + 2 * c4);
    out->ops.action = hp1 + oo_bytes + 3 * c4;
    out->ops.mark_type = hp1 + oo_bytes + 3 * c4 + c1;
    out->ops.values = (const uint32_t*)(hp1 + val_at);
    out->ops.n_values = n_replacement;
    out->ops.actor = nullptr;
    return PTX_OK;
}

ptx_status ptx_view_replace_plan(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, const uint32_t* replacement, uint32_t n_replacement,
                                 uint32_t n_batch_logs, ptx_replace_plan* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_status st = view_find_check(ctx, pattern, n_pattern, flags);
    if (st != PTX_OK) return st;
    if (n_replacement > PTX_CHANGE_ROWS_MAX) return fail(ctx, PTX_ERR_INVALID_ARG, "replacement of more than PTX_CHANGE_ROWS_MAX elements");
    if (n_replacement && !replacement) return fail(ctx, PTX_ERR_INVALID_ARG, "replacement is NULL");
    if ((uint64_t)n_batch_logs < (uint64_t)v->first_log + v->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "n_batch_logs ends before the view's range");
    ptx_host_result* h = new ptx_host_result();
    st = view_replace_impl(ctx, v, pattern, n_pattern, flags, replacement, n_replacement, n_batch_logs, h, out);
    if (st != PTX_OK) {
        delete h;
        memset(out, 0, sizeof(*out));
        return st;
    }
    out->owner = h;
    return PTX_OK;
}

ptx_status ptx_view_replace_plan_device(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, const uint32_t* replacement, uint32_t n_replacement,
                                        uint32_t n_batch_logs, const uint32_t* actor, uint32_t max_actors, ptx_replace_plan* counts, ptx_dinput_ops** ops) {
    if (!ctx || !v || !counts || !ops) return PTX_ERR_INVALID_ARG;
    memset(counts, 0, sizeof(*counts));
    *ops = nullptr;
    ptx_status st = view_find_check(ctx, pattern, n_pattern, flags);
    if (st != PTX_OK) return st;
    if (n_replacement > PTX_CHANGE_ROWS_MAX) return fail(ctx, PTX_ERR_INVALID_ARG, "replacement of more than PTX_CHANGE_ROWS_MAX elements");
    if (n_replacement && !replacement) return fail(ctx, PTX_ERR_INVALID_ARG, "replacement is NULL");
    if ((uint64_t)n_batch_logs < (uint64_t)v->first_log + v->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "n_batch_logs ends before the view's range");
    if (n_batch_logs && !actor) return fail(ctx, PTX_ERR_INVALID_ARG, "actor is NULL");
    ptx_host_result* h = new ptx_host_result();
    ptx_dinput_ops* d = new ptx_dinput_ops();
    st = view_replace_impl(ctx, v, pattern, n_pattern, flags, replacement, n_replacement, n_batch_logs, h, counts, d, actor, max_actors);
    if (st != PTX_OK) {
        delete h;
        delete d;
        memset(counts, 0, sizeof(*counts));
        return st;
    }
    counts->owner = h;
    *ops = d;
    return PTX_OK;
}

ptx_status ptx_view_text_slices(ptx_ctx* ctx, const ptx_dview* v, const uint64_t* slice_off, const uint32_t* slice_start, const uint32_t* slice_end, ptx_slices* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    const uint32_t n_logs = v->n_logs;
    if (n_logs && !slice_off) return fail(ctx, PTX_ERR_INVALID_ARG, "slice_off is NULL");
    if (n_logs && slice_off[0] != 0) return fail(ctx, PTX_ERR_INVALID_ARG, "slice_off[0] is not 0");
    for (uint32_t l = 0; l < n_logs; ++l)
        if (slice_off[l + 1] < slice_off[l]) return fail(ctx, PTX_ERR_INVALID_ARG, "slice_off decreases");
    const uint64_t ns64 = n_logs ? slice_off[n_logs] : 0;
    if (ns64 > 0xFFFFFFFFull) return fail(ctx, PTX_ERR_INVALID_ARG, "more than 2^32 - 1 slices");
    if (ns64 && (!slice_start || !slice_end)) return fail(ctx, PTX_ERR_INVALID_ARG, "slices present but slice_start or slice_end is NULL");
    const uint32_t ns = (uint32_t)ns64;
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_result* h = new ptx_host_result();
    const uint64_t no = (uint64_t)n_logs + 1, nso = ns64 + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status (the host's only) | elem_start | elem_end | unit_off, sspan_off — what comes down — | slice_off | slice_start |
     * slice_end — what goes up —; the device's goes on with slice_log | first_span | src_off */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), col = a16(ns64 * 4), es_at = st_bytes, ee_at = es_at + col, oo_at = ee_at + col, down0 = oo_at + a16(2 * nso * 8);
    const uint64_t so_at = down0, ss_at = so_at + a16(no * 8), se_at = ss_at + col, up_end = se_at + col, hblk0 = up_end + 16;
    const uint64_t sl_at = up_end, fs_at = sl_at + col, src_at = fs_at + col, dblk0 = src_at + a16(ns64 * 8) + 16;
    uint8_t *hp0 = nullptr, *d0 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, hblk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess && ns) e = ptx_dev_malloc((void**)&d0, dblk0);
    uint64_t* out_off = (uint64_t*)(hp0 + oo_at);
    float ms[2] = {0.f, 0.f};
    uint64_t out_units = 0, out_rows = 0, ot_bytes = 0, os_bytes = 0;
    PtxSliceArgs A;
    memset(&A, 0, sizeof(A));
    if (e == hipSuccess) {
        if (n_logs) memcpy(hp0, v->h_status.data(), (size_t)n_logs * 4);
        out_off[0] = out_off[nso] = 0; /* no slices: unit_off = sspan_off = {0} */
    }
    if (e == hipSuccess && ns) {
        view_text_args(v, A.T);
        A.slice_off = (const uint64_t*)(d0 + so_at);
        A.slice_start = (const uint32_t*)(d0 + ss_at);
        A.slice_end = (const uint32_t*)(d0 + se_at);
        A.n_slices = ns;
        A.pre_off = v->pre_off;
        A.pre = v->pre;
        A.elem_start = (uint32_t*)(d0 + es_at);
        A.elem_end = (uint32_t*)(d0 + ee_at);
        A.out_off = (uint64_t*)(d0 + oo_at);
        A.slice_log = (uint32_t*)(d0 + sl_at);
        A.first_span = (uint32_t*)(d0 + fs_at);
        A.src_off = (uint64_t*)(d0 + src_at);
        /* the caller's arrays are free to go */
        memcpy(hp0 + so_at, slice_off, (size_t)no * 8);
        memcpy(hp0 + ss_at, slice_start, (size_t)ns * 4);
        memcpy(hp0 + se_at, slice_end, (size_t)ns * 4);
        e = hipMemcpyAsync(d0 + so_at, hp0 + so_at, up_end - so_at, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_slice_bounds_kernel, dim3((uint32_t)((ns64 + 255) / 256)), dim3(256), 0, ctx->stream, A);
            hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.out_off, ns);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + es_at, d0 + es_at, down0 - es_at, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) {
            out_units = out_off[ns];
            out_rows = out_off[nso + ns];
        }
    }
    if (e == hipSuccess) e = slice_emit_passes(ctx, A, out_units, out_rows, h, 1, &ot_bytes, &os_bytes, &ms[1]);
    (void)ptx_dev_free(d0);
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("view slices: ") + hipGetErrorString(e));
    }
    const uint8_t* hp1 = (const uint8_t*)h->pinned[1];
    out->n_logs = n_logs;
    out->n_slices = ns;
    out->kernel_ms = ms[0] + ms[1];
    out->status = (const uint32_t*)hp0;
    out->elem_start = (const uint32_t*)(hp0 + es_at);
    out->elem_end = (const uint32_t*)(hp0 + ee_at);
    out->unit_off = out_off;
    out->sspan_off = out_off + nso;
    out->text = (const uint16_t*)hp1;
    out->sspans = (const ptx_span*)(hp1 + ot_bytes);
    out->sspan_unit = (const uint32_t*)(hp1 + ot_bytes + os_bytes);
    out->owner = h;
    return PTX_OK;
}

/* ---- queries by format on a view (markrun_core.h): count -> scan -> the number of listed runs comes down -> emit -> finish (-> bounds -> scan -> the slice
 *      passes).  ptx_view_mark_runs has two waits, ptx_view_mark_snippets three; ptx_view_find_in_marks keeps the uncapped runs on the device and runs the view's
 *      hit passes and the filter over them: four waits (runs, hits, kept hits, the answer) ---- */
struct ptx_host_mark_snippets {
    ptx_host_result runs, cut;
};

void ptx_mark_runs_free(ptx_mark_runs* m) {
    if (!m) return;
    delete (ptx_host_result*)m->owner;
    memset(m, 0, sizeof(*m));
}

void ptx_mark_snippets_free(ptx_mark_snippets* m) {
    if (!m) return;
    delete (ptx_host_mark_snippets*)m->owner;
    memset(m, 0, sizeof(*m));
}

static ptx_status view_mark_check(ptx_ctx* ctx, uint32_t mark_type, uint32_t id, bool find) {
    if (mark_type != PTX_MARK_STRONG && mark_type != PTX_MARK_EM && mark_type != PTX_MARK_COMMENT && mark_type != PTX_MARK_LINK)
        return fail(ctx, PTX_ERR_INVALID_ARG, "unknown mark type");
    if ((mark_type == PTX_MARK_STRONG || mark_type == PTX_MARK_EM) && id != PTX_MARK_ANY_ID) return fail(ctx, PTX_ERR_INVALID_ARG, "strong and em take PTX_MARK_ANY_ID");
    if (mark_type == PTX_MARK_LINK && id != PTX_MARK_ANY_ID && id > PTX_ATTR_ID_MASK) return fail(ctx, PTX_ERR_INVALID_ARG, "url id beyond PTX_ATTR_ID_MASK");
    if (find && mark_type == PTX_MARK_COMMENT && id == PTX_MARK_ANY_ID)
        return fail(ctx, PTX_ERR_INVALID_ARG, "a find inside comments needs one comment id: intervals of different ids are not sorted by start");
    return PTX_OK;
}

enum { PTX_MARKS_RUNS = 0, PTX_MARKS_SNIPPETS = 1, PTX_MARKS_DEVICE = 2 };
/* PTX_MARKS_DEVICE: the listed runs stay where the passes left them; the caller gives both blocks back to the pool */
struct ptx_mark_runs_keep {
    uint8_t *d0 = nullptr, *d1 = nullptr;
    const uint64_t* run_off = nullptr; /* device [n_logs + 1] */
    const uint32_t *run_start = nullptr, *run_end = nullptr;
    float ms = 0.f;
};

/* THE run sequence of all three entry points; the arguments are checked.  h->pinned[0]: status | n_runs | run_off,  h->pinned[1]: run_start | run_end | run_id |
 * run_unit | run_len and, for snippets, | elem_start | elem_end | match_unit | unit_off, sspan_off;  cut->pinned[0]: text | sspans | sspan_unit */
static ptx_status view_marks_impl(ptx_ctx* ctx, const ptx_dview* v, uint32_t mark_type, uint32_t id, uint32_t cap, int mode, uint32_t before, uint32_t after, ptx_host_result* h,
                                  ptx_host_result* cut, ptx_mark_snippets* out, ptx_mark_runs_keep* keep) {
    PTX_HIP(ctx, ptx_enter(ctx));
    const bool snip = mode == PTX_MARKS_SNIPPETS, dev = mode == PTX_MARKS_DEVICE;
    const uint32_t n_logs = v->n_logs;
    const uint64_t no = (uint64_t)n_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status (the host's only: the view keeps the device's) | n_runs | run_off (two rows: the scan kernel's) */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), ro_at = 2 * st_bytes, blk0 = ro_at + a16(2 * no * 8);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, blk0, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess && n_logs) e = ptx_dev_malloc((void**)&d0, blk0);
    uint64_t* run_off = (uint64_t*)(hp0 + ro_at);
    float ms[3] = {0.f, 0.f, 0.f};
    uint64_t nr = 0, out_units = 0, out_rows = 0, ot_bytes = 0, os_bytes = 0;
    bool too_many = false;
    PtxMarkRunArgs A;
    memset(&A, 0, sizeof(A));
    if (e == hipSuccess) {
        if (n_logs) memcpy(hp0, v->h_status.data(), (size_t)n_logs * 4);
        run_off[0] = 0; /* an empty view: run_off = {0} */
    }
    if (e == hipSuccess && n_logs) {
        A.log_off = v->log_off;
        A.spans = v->r->spans;
        A.cints = v->r->cints;
        A.logs = v->r->logs;
        A.status = v->status;
        A.span_off = v->off + no;
        A.pre_off = v->pre_off;
        A.pre = v->pre;
        A.first_log = v->first_log;
        A.n_logs = n_logs;
        A.mark_type = mark_type;
        A.id = id;
        A.cap = cap;
        A.before = before;
        A.after = after;
        A.n_runs = (uint32_t*)(d0 + st_bytes);
        A.run_off = (uint64_t*)(d0 + ro_at);
        e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_markrun_count_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, A.run_off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + st_bytes, d0 + st_bytes, st_bytes + no * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) nr = run_off[n_logs];
        if (e == hipSuccess && nr > 0xFFFFFFFFull) too_many = true, e = hipErrorInvalidValue; /* a lane per listed run, a slice per run */
    }
    /* block 1, device and pinned host alike: run_start | run_end | run_id | run_unit | run_len and, for snippets, | elem_start | elem_end | match_unit | unit_off,
     * sspan_off — all of it comes down in one copy, nothing goes up —; the device's goes on with win_start | win_end | slice_log | first_span | src_off */
    const uint64_t nso = nr + 1, col = a16(nr * 4), oo_at = (snip ? 8 : 5) * col, down1 = oo_at + (snip ? a16(2 * nso * 8) : 0), hblk1 = down1 + 16;
    const uint64_t ws_at = down1, sl_at = ws_at + 2 * col, src_at = sl_at + 2 * col, dblk1 = snip ? src_at + a16(nr * 8) + 16 : hblk1;
    if (e == hipSuccess && !dev) e = hipHostMalloc((void**)&hp1, hblk1, hipHostMallocDefault);
    h->pinned[1] = hp1;
    uint64_t* out_off = (uint64_t*)(hp1 + oo_at);
    if (e == hipSuccess && snip) out_off[0] = out_off[nso] = 0; /* no runs: unit_off = sspan_off = {0} */
    PtxSliceArgs S;
    memset(&S, 0, sizeof(S));
    if (e == hipSuccess && nr) {
        e = ptx_dev_malloc((void**)&d1, dblk1);
        if (e == hipSuccess) {
            A.n_listed = (uint32_t)nr;
            A.run_start = (uint32_t*)d1;
            A.run_end = (uint32_t*)(d1 + col);
            A.run_id = (uint32_t*)(d1 + 2 * col);
            A.run_unit = (uint32_t*)(d1 + 3 * col);
            A.run_len = (uint32_t*)(d1 + 4 * col);
            if (snip) {
                A.match_unit = (uint32_t*)(d1 + 7 * col);
                A.win_start = (uint32_t*)(d1 + ws_at);
                A.win_end = (uint32_t*)(d1 + ws_at + col);
                view_text_args(v, S.T);
                S.slice_off = A.run_off; /* one slice per listed run, in run order */
                S.slice_start = A.win_start;
                S.slice_end = A.win_end;
                S.n_slices = (uint32_t)nr;
                S.pre_off = v->pre_off;
                S.pre = v->pre;
                S.elem_start = (uint32_t*)(d1 + 5 * col);
                S.elem_end = (uint32_t*)(d1 + 6 * col);
                S.out_off = (uint64_t*)(d1 + oo_at);
                S.slice_log = (uint32_t*)(d1 + sl_at);
                S.first_span = (uint32_t*)(d1 + sl_at + col);
                S.src_off = (uint64_t*)(d1 + src_at);
            }
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            const uint32_t grid = (uint32_t)((nr + 255) / 256);
            hipLaunchKernelGGL(ptx_markrun_emit_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, A);
            if (!dev) hipLaunchKernelGGL(ptx_markrun_finish_kernel, dim3(grid), dim3(256), 0, ctx->stream, A);
            if (snip) {
                hipLaunchKernelGGL(ptx_slice_bounds_kernel, dim3(grid), dim3(256), 0, ctx->stream, S);
                hipLaunchKernelGGL(ptx_text_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, S.out_off, (uint32_t)nr);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess && !dev) e = hipMemcpyAsync(hp1, d1, snip ? oo_at + 2 * nso * 8 : 5 * col, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
        if (e == hipSuccess && snip) {
            out_units = out_off[nr];
            out_rows = out_off[nso + nr];
        }
    }
    if (e == hipSuccess && snip) e = slice_emit_passes(ctx, S, out_units, out_rows, cut, 0, &ot_bytes, &os_bytes, &ms[2]);
    if (e != hipSuccess || !dev) {
        (void)ptx_dev_free(d0);
        (void)ptx_dev_free(d1);
    }
    if (e != hipSuccess) {
        if (too_many) return fail(ctx, PTX_ERR_CAPACITY, "more than 2^32 - 1 listed runs: lower max_runs_per_log or the range");
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("view marks: ") + hipGetErrorString(e));
    }
    if (dev) {
        keep->d0 = d0;
        keep->d1 = d1;
        keep->run_off = A.run_off;
        keep->run_start = A.run_start;
        keep->run_end = A.run_end;
        keep->ms = ms[0] + ms[1];
        return PTX_OK;
    }
    out->n_logs = n_logs;
    out->mark_type = mark_type;
    out->kernel_ms = ms[0] + ms[1] + ms[2];
    out->n_slices = snip ? (uint32_t)nr : 0u;
    out->status = (const uint32_t*)hp0;
    out->n_runs = (const uint32_t*)(hp0 + st_bytes);
    out->run_off = run_off;
    out->run_start = (const uint32_t*)hp1;
    out->run_end = (const uint32_t*)(hp1 + col);
    out->run_id = (const uint32_t*)(hp1 + 2 * col);
    out->run_unit = (const uint32_t*)(hp1 + 3 * col);
    out->run_len = (const uint32_t*)(hp1 + 4 * col);
    if (snip) {
        const uint8_t* hp2 = (const uint8_t*)cut->pinned[0];
        out->elem_start = (const uint32_t*)(hp1 + 5 * col);
        out->elem_end = (const uint32_t*)(hp1 + 6 * col);
        out->match_unit = (const uint32_t*)(hp1 + 7 * col);
        out->unit_off = out_off;
        out->sspan_off = out_off + nso;
        out->text = (const uint16_t*)hp2;
        out->sspans = (const ptx_span*)(hp2 + ot_bytes);
        out->sspan_unit = (const uint32_t*)(hp2 + ot_bytes + os_bytes);
    }
    return PTX_OK;
}

ptx_status ptx_view_mark_runs(ptx_ctx* ctx, const ptx_dview* v, uint32_t mark_type, uint32_t id, uint32_t max_runs_per_log, ptx_mark_runs* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_status st = view_mark_check(ctx, mark_type, id, false);
    if (st != PTX_OK) return st;
    ptx_host_result* h = new ptx_host_result();
    ptx_mark_snippets m;
    memset(&m, 0, sizeof(m));
    st = view_marks_impl(ctx, v, mark_type, id, max_runs_per_log, PTX_MARKS_RUNS, 0u, 0u, h, nullptr, &m, nullptr);
    if (st != PTX_OK) {
        delete h;
        return st;
    }
    out->n_logs = m.n_logs;
    out->mark_type = m.mark_type;
    out->kernel_ms = m.kernel_ms;
    out->status = m.status;
    out->n_runs = m.n_runs;
    out->run_off = m.run_off;
    out->run_start = m.run_start;
    out->run_end = m.run_end;
    out->run_id = m.run_id;
    out->run_unit = m.run_unit;
    out->run_len = m.run_len;
    out->owner = h;
    return PTX_OK;
}

ptx_status ptx_view_mark_snippets(ptx_ctx* ctx, const ptx_dview* v, uint32_t mark_type, uint32_t id, uint32_t max_runs_per_log, uint32_t before, uint32_t after,
                                  ptx_mark_snippets* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_status st = view_mark_check(ctx, mark_type, id, false);
    if (st != PTX_OK) return st;
    ptx_host_mark_snippets* h = new ptx_host_mark_snippets();
    st = view_marks_impl(ctx, v, mark_type, id, max_runs_per_log, PTX_MARKS_SNIPPETS, before, after, &h->runs, &h->cut, out, nullptr);
    if (st != PTX_OK) {
        delete h;
        memset(out, 0, sizeof(*out));
        return st;
    }
    out->owner = h;
    return PTX_OK;
}

/* the view's hit passes, uncapped, into scratch; the filter over the runs `K` holds; the kept hits down.  h->pinned[0]: status | n_matches | hit_off,
 * h->pinned[1]: hit_unit | hit_start | hit_end */
static ptx_status view_find_in_marks_impl(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log,
                                          const ptx_mark_runs_keep& K, ptx_host_result* h, ptx_matches* out) {
    PTX_HIP(ctx, ptx_enter(ctx));
    const uint32_t n_logs = v->n_logs;
    const uint64_t no = (uint64_t)n_logs + 1;
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    /* block 0, device and pinned host alike: status (the host's only) | n_matches | hit_off — what comes down — | the pattern; the device's goes on with the
     * uncapped counts and their offsets */
    const uint64_t st_bytes = a16((uint64_t)n_logs * 4), down0 = 2 * st_bytes + a16(no * 8), pat_at = down0, hblk0 = pat_at + a16((uint64_t)n_pattern * 2);
    const uint64_t na_at = hblk0, ao_at = na_at + st_bytes, dblk0 = ao_at + a16(no * 8);
    uint8_t *hp0 = nullptr, *hp1 = nullptr, *d0 = nullptr, *d1 = nullptr, *d2 = nullptr;
    hipError_t e = hipHostMalloc((void**)&hp0, hblk0 + 16, hipHostMallocDefault);
    h->pinned[0] = hp0;
    if (e == hipSuccess && n_logs) e = ptx_dev_malloc((void**)&d0, dblk0);
    uint64_t* hit_off = (uint64_t*)(hp0 + 2 * st_bytes);
    uint64_t* total = (uint64_t*)(hp0 + hblk0); /* the uncapped hits of the view */
    float ms[3] = {0.f, 0.f, 0.f};
    uint64_t nall = 0, nkept = 0;
    bool too_many = false;
    PtxViewArgs V;
    PtxMarkFilterArgs F;
    memset(&V, 0, sizeof(V));
    memset(&F, 0, sizeof(F));
    if (e == hipSuccess) {
        if (n_logs) memcpy(hp0, v->h_status.data(), (size_t)n_logs * 4);
        memcpy(hp0 + pat_at, pattern, (size_t)n_pattern * 2); /* the caller's pattern is free to go */
        hit_off[0] = 0;                                       /* an empty view: hit_off = {0} */
        *total = 0;
    }
    if (e == hipSuccess && n_logs) {
        view_text_args(v, V.F.T);
        V.F.n_matches = (uint32_t*)(d0 + na_at);
        V.F.hit_off = (uint64_t*)(d0 + ao_at);
        V.F.pattern = (const uint16_t*)(d0 + pat_at);
        V.F.n_pattern = n_pattern;
        V.F.flags = flags;
        V.F.cap = 0xFFFFFFFFu;
        V.pre_off = v->pre_off;
        V.pre = v->pre;
        e = hipMemcpyAsync(d0 + pat_at, hp0 + pat_at, (size_t)n_pattern * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_find_count_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, V.F);
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)V.F.n_matches, 0xFFFFFFFFu, V.F.hit_off, n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(total, V.F.hit_off + n_logs, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) nall = *total;
        if (e == hipSuccess && nall > 0xFFFFFFFFull) too_many = true, e = hipErrorInvalidValue; /* a lane per hit */
    }
    /* block 1, device only: hit_unit | hit_start | hit_end of ALL hits */
    const uint64_t cola = a16(nall * 4);
    if (e == hipSuccess && n_logs) {
        if (nall) e = ptx_dev_malloc((void**)&d1, 3 * cola + 16);
        if (e == hipSuccess) {
            V.n_hits = (uint32_t)nall;
            V.F.hit_unit = (uint32_t*)d1;
            V.F.hit_start = (uint32_t*)(d1 + cola);
            V.F.hit_end = (uint32_t*)(d1 + 2 * cola);
            F.n_logs = n_logs;
            F.cap = max_hits_per_log;
            F.hit_off = V.F.hit_off;
            F.hit_unit = V.F.hit_unit;
            F.hit_start = V.F.hit_start;
            F.hit_end = V.F.hit_end;
            F.run_off = K.run_off;
            F.run_start = K.run_start;
            F.run_end = K.run_end;
            F.n_kept = (uint32_t*)(d0 + st_bytes);
            F.out_off = (const uint64_t*)(d0 + 2 * st_bytes);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            if (nall) {
                hipLaunchKernelGGL(ptx_view_positions_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, V.F);
                hipLaunchKernelGGL(ptx_view_locate_kernel, dim3((uint32_t)((nall + 255) / 256)), dim3(256), 0, ctx->stream, V);
            }
            hipLaunchKernelGGL(ptx_markrun_filter_count_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, F); /* (a view without a hit: zeros) */
            hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)F.n_kept, max_hits_per_log, (uint64_t*)(d0 + 2 * st_bytes), n_logs);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp0 + st_bytes, d0 + st_bytes, down0 - st_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ctx->ev0, ctx->ev1);
        if (e == hipSuccess) nkept = hit_off[n_logs];
    }
    /* block 2, device and pinned host alike: hit_unit | hit_start | hit_end of the listed kept hits */
    const uint64_t col = a16(nkept * 4);
    if (e == hipSuccess) e = hipHostMalloc((void**)&hp1, 3 * col + 16, hipHostMallocDefault);
    h->pinned[1] = hp1;
    if (e == hipSuccess && nkept) {
        e = ptx_dev_malloc((void**)&d2, 3 * col + 16);
        if (e == hipSuccess) {
            F.out_unit = (uint32_t*)d2;
            F.out_start = (uint32_t*)(d2 + col);
            F.out_end = (uint32_t*)(d2 + 2 * col);
            e = hipEventRecord(ctx->ev0, ctx->stream);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ptx_markrun_filter_emit_kernel, dim3(n_logs), dim3(64), 0, ctx->stream, F);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hp1, d2, 3 * col, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[2], ctx->ev0, ctx->ev1);
    }
    (void)ptx_dev_free(d0);
    (void)ptx_dev_free(d1);
    (void)ptx_dev_free(d2);
    if (e != hipSuccess) {
        if (too_many) return fail(ctx, PTX_ERR_CAPACITY, "more than 2^32 - 1 matches in the view: narrow the range");
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("view find in marks: ") + hipGetErrorString(e));
    }
    out->n_logs = n_logs;
    out->n_pattern = n_pattern;
    out->kernel_ms = K.ms + ms[0] + ms[1] + ms[2];
    out->status = (const uint32_t*)hp0;
    out->n_matches = (const uint32_t*)(hp0 + st_bytes);
    out->hit_off = hit_off;
    out->hit_unit = (const uint32_t*)hp1;
    out->hit_start = (const uint32_t*)(hp1 + col);
    out->hit_end = (const uint32_t*)(hp1 + 2 * col);
    return PTX_OK;
}

ptx_status ptx_view_find_in_marks(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t mark_type, uint32_t id,
                                  uint32_t max_hits_per_log, ptx_matches* out) {
    if (!ctx || !v || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_status st = view_find_check(ctx, pattern, n_pattern, flags);
    if (st == PTX_OK) st = view_mark_check(ctx, mark_type, id, true);
    if (st != PTX_OK) return st;
    ptx_mark_runs_keep K;
    {
        ptx_host_result tmp; /* the runs' counts: nobody asks for them */
        st = view_marks_impl(ctx, v, mark_type, id, 0xFFFFFFFFu, PTX_MARKS_DEVICE, 0u, 0u, &tmp, nullptr, nullptr, &K);
    }
    if (st != PTX_OK) return st;
    ptx_host_result* h = new ptx_host_result();
    st = view_find_in_marks_impl(ctx, v, pattern, n_pattern, flags, max_hits_per_log, K, h, out);
    (void)ptx_dev_free(K.d0);
    (void)ptx_dev_free(K.d1);
    if (st != PTX_OK) {
        delete h;
        memset(out, 0, sizeof(*out));
        return st;
    }
    out->owner = h;
    return PTX_OK;
}

ptx_status ptx_result_download_logs(ptx_ctx* ctx, const ptx_dresult* r, ptx_log_result* out, uint32_t n_logs) {
    if (!ctx || !r || (!out && n_logs)) return PTX_ERR_INVALID_ARG;
    if (n_logs > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "n_logs exceeds the result");
    PTX_HIP(ctx, ptx_enter(ctx));
    if (n_logs) PTX_HIP(ctx, hipMemcpyAsync(out, r->logs, (size_t)n_logs * sizeof(ptx_log_result), hipMemcpyDeviceToHost, ctx->stream));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PTX_OK;
}

const ptx_log_result* ptx_dresult_logs_device(const ptx_dresult* r) { return r ? r->logs : nullptr; }

ptx_status ptx_pack_digests(ptx_ctx* ctx, const ptx_dresult* r, uint32_t first, uint32_t count, uint64_t* dst_device) {
    if (!ctx || !r || (!dst_device && count)) return PTX_ERR_INVALID_ARG;
    if ((uint64_t)first + count > r->n_logs) return fail(ctx, PTX_ERR_INVALID_ARG, "digest range exceeds the result");
    PTX_HIP(ctx, ptx_enter(ctx));
    if (count) {
        hipLaunchKernelGGL(ptx_pack_digests_kernel, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, r->logs, first, count, dst_device);
        PTX_HIP(ctx, hipGetLastError());
    }
    return PTX_OK;
}

ptx_status ptx_apply_materialize(ptx_ctx* ctx, const ptx_batch* batch, ptx_result* out) {
    if (!ctx || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    ptx_dbatch* b = nullptr;
    ptx_dresult* r = nullptr;
    ptx_status st = upload_tiled(ctx, batch, 1, &b, false); /* merged once: an index would be written and never read */
    if (st == PTX_OK) st = ptx_result_alloc(ctx, b, &r);
    if (st == PTX_OK) st = ptx_merge(ctx, b, r);
    if (st == PTX_OK) st = ptx_result_download(ctx, b, r, out);
    ptx_dresult_free(ctx, r);
    ptx_batch_free(ctx, b);
    return st;
}

/* ---- patch streams ---- */
struct ptx_host_patches {
    std::vector<uint64_t> off;
    std::vector<ptx_patch_log> logs;
    std::vector<ptx_patch> patches;
};

void ptx_patches_free(ptx_patches* p) {
    if (!p) return;
    delete (ptx_host_patches*)p->owner;
    memset(p, 0, sizeof(*p));
}

ptx_status ptx_replay_patches(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, ptx_patches* out) { return ptx_replay_patches_from(ctx, b, r, nullptr, out); }

/* who takes the packed records of a replay instead of the host (ptx_check_patches): the accumulate kernels, on every packed range while it sits on the device */
struct PtxAccumSink {
    const ptx_dresult* want;      /* the merge's result the streams are compared with */
    ptx_patch_check_log* d_check; /* device [n_logs] */
    float accum_ms;               /* HIP-event time of the accumulate launches, summed over the ranges */
};
/* the device blocks of the accumulate launches: made once per call, for its largest range (the chunked pack path has a range per few logs) */
struct PtxAccumScratch {
    uint32_t *d_idx = nullptr, *d_state = nullptr;
    uint64_t* d_soff = nullptr;
    uint64_t idx_cap = 0, state_units = 0;
};
static void accum_scratch_free(PtxAccumScratch* sc) {
    (void)ptx_dev_free(sc->d_idx);
    (void)ptx_dev_free(sc->d_state);
    (void)ptx_dev_free(sc->d_soff);
    *sc = PtxAccumScratch();
}
/* which state store a log takes: the slice of global scratch where its state exceeds one CU's LDS — or always, PTX_FLAG_ACCUM_HBM_STATE */
static bool accum_log_to_hbm(const ptx_ctx* ctx, uint64_t rows, const ptx_log_hdr& h) { return (ctx->flags & PTX_FLAG_ACCUM_HBM_STATE) != 0 || ptx_accum_lds_need_hdr(rows, h) > ctx->max_lds; }
static uint64_t accum_slice_units(uint64_t rows, const ptx_log_hdr& h) { return (ptx_accum_units_hdr(rows, h) + 31u) & ~31ull; } /* (slices do not share a cache line) */
/* room for the logs [l0, l1): never shrinks; a call that knows its ranges asks for the largest first */
static hipError_t accum_scratch_reserve(PtxAccumScratch* sc, uint64_t n_logs, uint64_t state_units) {
    hipError_t e = hipSuccess;
    if (n_logs > sc->idx_cap) {
        (void)ptx_dev_free(sc->d_idx);
        (void)ptx_dev_free(sc->d_soff);
        sc->d_idx = nullptr, sc->d_soff = nullptr, sc->idx_cap = 0;
        e = ptx_dev_malloc((void**)&sc->d_idx, n_logs * 4);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&sc->d_soff, (n_logs + 1) * 8);
        if (e == hipSuccess) sc->idx_cap = n_logs;
    }
    if (e == hipSuccess && state_units > sc->state_units) {
        (void)ptx_dev_free(sc->d_state);
        sc->d_state = nullptr, sc->state_units = 0;
        e = ptx_dev_malloc((void**)&sc->d_state, 4 * state_units + 128);
        if (e == hipSuccess) sc->state_units = state_units;
    }
    return e;
}
static uint64_t accum_range_state_units(const ptx_ctx* ctx, const std::vector<ptx_log_hdr>& hdr, const std::vector<uint64_t>& log_off, uint32_t l0, uint32_t l1) {
    uint64_t units = 0;
    for (uint32_t l = l0; l < l1; ++l)
        if (accum_log_to_hbm(ctx, log_off[l + 1] - log_off[l], hdr[l])) units += accum_slice_units(log_off[l + 1] - log_off[l], hdr[l]);
    return units;
}
/* The accumulate launches for the logs [l0, l1): those whose state fits the LDS in one launch of ptx_accum_kernel (its window = the largest of them), the others
 * — or all, PTX_FLAG_ACCUM_HBM_STATE — in one of ptx_accum_kernel_hbm with a state slice each.  A = everything but the launch's own fields.  Waits for the
 * stream (the caller fills the record buffer and this scratch again); *ms += the launches' HIP-event time when asked for (the context's two events: the
 * replay's time has been read by then). */
static ptx_status accum_launch_range(ptx_ctx* ctx, PtxAccumScratch* sc, const std::vector<ptx_log_hdr>& hdr, const std::vector<uint64_t>& log_off, uint32_t l0, uint32_t l1, PtxAccumArgs A,
                                     float* ms) {
    if (l1 <= l0) return PTX_OK;
    std::vector<uint32_t> lds_logs, hbm_logs;
    std::vector<uint64_t> soff(1, 0);
    uint64_t need = 0;
    for (uint32_t l = l0; l < l1; ++l) {
        const uint64_t rows = log_off[l + 1] - log_off[l];
        if (accum_log_to_hbm(ctx, rows, hdr[l])) {
            hbm_logs.push_back(l);
            soff.push_back(soff.back() + accum_slice_units(rows, hdr[l]));
        } else {
            lds_logs.push_back(l);
            need = std::max(need, ptx_accum_lds_need_hdr(rows, hdr[l]));
        }
    }
    const uint32_t n_lds = (uint32_t)lds_logs.size(), n_hbm = (uint32_t)hbm_logs.size();
    const uint32_t lds_bytes = (uint32_t)std::min<uint64_t>((need + 255) & ~255ull, ctx->max_lds);
    std::vector<uint32_t> idx(lds_logs);
    idx.insert(idx.end(), hbm_logs.begin(), hbm_logs.end());
    hipError_t e = accum_scratch_reserve(sc, idx.size(), soff[n_hbm]);
    if (e == hipSuccess) e = hipMemcpyAsync(sc->d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n_hbm) e = hipMemcpyAsync(sc->d_soff, soff.data(), ((size_t)n_hbm + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && ms) e = hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess && n_lds) {
        A.first_log = 0;
        A.n_launch = n_lds;
        A.log_index = sc->d_idx;
        A.state = nullptr;
        A.state_off = nullptr;
        A.lds_bytes = lds_bytes;
        hipLaunchKernelGGL(ptx_accum_kernel, dim3(n_lds), dim3(64), lds_bytes, ctx->stream, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_hbm) {
        A.first_log = 0;
        A.n_launch = n_hbm;
        A.log_index = sc->d_idx + n_lds;
        A.state = (uint32_t*)(((uintptr_t)sc->d_state + 127u) & ~(uintptr_t)127u);
        A.state_off = sc->d_soff;
        A.lds_bytes = PTX_ACCUM_HBM_LDS_BYTES;
        hipLaunchKernelGGL(ptx_accum_kernel_hbm, dim3(n_hbm), dim3(64), 0, ctx->stream, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && ms) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); /* (idx / soff are pageable host memory of this frame, and the caller reuses the blocks) */
    if (e == hipSuccess && ms) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, ctx->ev0, ctx->ev1) == hipSuccess) *ms += t;
    }
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_accum_kernel: ") + hipGetErrorString(e));
    return PTX_OK;
}

static ptx_status replay_patches_impl(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const uint32_t* first_row, ptx_patches* out, PtxAccumSink* sink);
ptx_status ptx_replay_patches_from(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const uint32_t* first_row, ptx_patches* out) {
    return replay_patches_impl(ctx, b, r, first_row, out, nullptr);
}

/* the replay; with a sink the packed records of every range go to the accumulate kernels instead of the host: no record download, no host room for them */
static ptx_status replay_patches_impl(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const uint32_t* first_row, ptx_patches* out, PtxAccumSink* sink) {
    if (!ctx || !b || !r || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if (!r->rank) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_replay_patches needs the elem_rank column (context created with PTX_FLAG_NO_ELEM_RANK)");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_patches* h = new ptx_host_patches();
    const uint32_t L = b->n_logs;
    h->off.assign((size_t)L + 1, 0);
    h->logs.resize(std::max<uint32_t>(L, 1));
    out->owner = h;
    out->n_logs = L;
    if (L == 0) {
        h->patches.resize(1);
        out->patch_off = h->off.data();
        out->logs = h->logs.data();
        out->patches = h->patches.data();
        return PTX_OK;
    }
    /* launch shape from the log headers: LDS of the largest replay working set */
    std::vector<ptx_log_hdr> hdr(L);
    std::vector<uint64_t> log_off((size_t)L + 1);
    hipError_t e = hipMemcpyAsync(hdr.data(), b->log_hdr, (size_t)L * sizeof(ptx_log_hdr), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(log_off.data(), b->log_off, ((size_t)L + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ptx_patches_free(out);
        return fail(ctx, PTX_ERR_HIP, std::string("replay set-up: ") + hipGetErrorString(e));
    }
    uint64_t need = 0, need_g = 0;
    /* Logs whose replay state does not fit one CU's LDS — or every log, PTX_FLAG_REPLAY_HBM_STATE — go to ONE launch of ptx_replay_kernel_hbm over a list of
     * log indices (replay_hbm_core.h: the state in a slice of global scratch per log); the others take the launch below exactly as before, its shape (need, wide,
     * gwin) computed over them alone, so a giant neighbour costs them no occupancy.  A log of more than 32 766 elements whose result lacks the slots' high
     * halves reports PTX_ERR_CAPACITY from either kernel; it is listed for the HBM-state one, which refuses it before it touches anything. */
    const bool lds_only = (ctx->flags & PTX_FLAG_REPLAY_LDS_ONLY) != 0, no_hi = b->wide_slots && !r->refs_hi;
    std::vector<uint8_t> to_hbm(L, 0);
    for (uint32_t l = 0; l < L; ++l) {
        const bool wide_l = ptx_replay_wants_wide(log_off[l + 1] - log_off[l], hdr[l]);
        to_hbm[l] = (ctx->flags & PTX_FLAG_REPLAY_HBM_STATE) != 0 || (no_hi && hdr[l].n_ins > 32766u) || ptx_replay_lds_need_hdr(hdr[l], wide_l || !lds_only, wide_l) > ctx->max_lds;
    }
    /* round 6: a launch with a log of more than 32 766 list elements or 65 534 rows takes the wide build (32-bit ranks and slots; the slots' high halves come
     * from the merge: r->refs_hi, there whenever the census found such a log) */
    bool wide = false;
    for (uint32_t l = 0; l < L; ++l) wide = wide || (!to_hbm[l] && ptx_replay_wants_wide(log_off[l + 1] - log_off[l], hdr[l]));
    if (wide && no_hi) wide = false; /* (results allocated for another batch: such logs report PTX_ERR_CAPACITY as before) */
    if (wide) /* (a narrow log beside a wide one is replayed by the wide build: the few that fit only the narrow form go with the large ones) */
        for (uint32_t l = 0; l < L; ++l) to_hbm[l] = to_hbm[l] || ptx_replay_lds_need_hdr(hdr[l], true, true) > ctx->max_lds;
    std::vector<uint32_t> hbm_logs;
    for (uint32_t l = 0; l < L; ++l) {
        if (to_hbm[l]) {
            hbm_logs.push_back(l);
            continue;
        }
        need = std::max<uint64_t>(need, ptx_replay_lds_need_hdr(hdr[l], false, wide));
        need_g = std::max<uint64_t>(need_g, ptx_replay_lds_need_hdr(hdr[l], true, wide));
    }
    const uint32_t n_hbm = (uint32_t)hbm_logs.size(), n_lds = L - n_hbm;
    out->reserved = n_hbm;
    /* The replay is one wave per log and lives on occupancy.  Above PTX_REPLAY_GWIN_ABOVE bytes of working set the LDS, not the wave slots, bounds the resident
     * logs: the per-slot link urls and the tables of applied mark ops (half of it; read only by the few ops that need them) move to global memory. */
    const bool gwin = wide || (need > PTX_REPLAY_GWIN_ABOVE && !lds_only);
    if (gwin) need = need_g;
    const uint32_t lds_bytes = (uint32_t)std::min<uint64_t>((need + 255) & ~255ull, ctx->max_lds); /* (the logs of the other launch do not fit it: this one leaves them at once, PTX_ERR_CAPACITY, and the HBM-state launch BEHIND it on the stream writes their records, plogs and extents last) */
    uint16_t* d_win = nullptr;
    uint64_t* d_winoff = nullptr;
    uint32_t* d_first = nullptr;
    uint32_t *d_state = nullptr, *d_hidx = nullptr;
    uint64_t* d_soff = nullptr;
    auto release_setup = [&]() {
        (void)ptx_dev_free(d_win);
        (void)ptx_dev_free(d_winoff);
        (void)ptx_dev_free(d_first);
        (void)ptx_dev_free(d_state);
        (void)ptx_dev_free(d_hidx);
        (void)ptx_dev_free(d_soff);
    };
    if (gwin && n_lds) { /* every log's slice of the scratch: what its header says it needs (nothing for the logs of the other launch) */
        std::vector<uint64_t> woff((size_t)L + 1, 0);
        for (uint32_t l = 0; l < L; ++l) woff[l + 1] = woff[l] + (to_hbm[l] ? 0u : ptx_replay_win_units_hdr(hdr[l], wide));
        e = ptx_dev_malloc((void**)&d_win, 2 * woff[L] + 16);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_winoff, ((size_t)L + 1) * 8);
        if (e == hipSuccess) e = hipMemcpyAsync(d_winoff, woff.data(), ((size_t)L + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); /* (woff leaves scope) */
        if (e != hipSuccess) { /* (an early return here leaked the offsets already held by `out`, and named an out-of-memory PTX_ERR_HIP) */
            release_setup();
            ptx_patches_free(out);
            return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("replay set-up (scratch): ") + hipGetErrorString(e));
        }
    }
    if (n_hbm) { /* the state slices of the HBM-state launch (the kernel zeroes what it needs zeroed) */
        std::vector<uint64_t> soff((size_t)n_hbm + 1, 0);
        for (uint32_t k = 0; k < n_hbm; ++k) soff[k + 1] = soff[k] + ptx_replay_hbm_units_hdr(hdr[hbm_logs[k]]);
        e = ptx_dev_malloc((void**)&d_state, 4 * soff[n_hbm] + 16);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_soff, ((size_t)n_hbm + 1) * 8);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_hidx, (size_t)n_hbm * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(d_soff, soff.data(), ((size_t)n_hbm + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_hidx, hbm_logs.data(), (size_t)n_hbm * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); /* (soff leaves scope) */
        if (e != hipSuccess) {
            release_setup();
            ptx_patches_free(out);
            return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("replay set-up (state scratch): ") + hipGetErrorString(e));
        }
    }
    if (first_row) {
        e = ptx_dev_malloc((void**)&d_first, (size_t)L * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(d_first, first_row, (size_t)L * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            release_setup();
            ptx_patches_free(out);
            return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("replay set-up: ") + hipGetErrorString(e));
        }
    }
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t n = log_off[l + 1] - log_off[l], skip = first_row ? std::min<uint64_t>(first_row[l], n) : 0;
        h->off[l + 1] = h->off[l] + 2 * (n - skip) + 16; /* the guess: two records per row asked for */
    }

    uint64_t *d_off = nullptr, *d_ext = nullptr, *d_xoff = nullptr;
    unsigned long long* d_next = nullptr;
    ptx_patch_log* d_logs = nullptr;
    ptx_patch *d_patches = nullptr, *d_packed = nullptr;
    ptx_status st = PTX_OK;
    auto release = [&]() {
        (void)ptx_dev_free(d_off);
        (void)ptx_dev_free(d_ext);
        (void)ptx_dev_free(d_xoff);
        (void)ptx_dev_free(d_next);
        (void)ptx_dev_free(d_logs);
        (void)ptx_dev_free(d_patches);
        (void)ptx_dev_free(d_packed);
        d_off = d_ext = d_xoff = nullptr;
        d_next = nullptr;
        d_logs = nullptr;
        d_patches = d_packed = nullptr;
    };
    /* ONE launch: every log writes into its guessed capacity; a log that outgrows it takes one overflow extent from an arena behind the capacities (an atomic
     * bump inside the kernel) and goes on there; a small kernel then packs the records of every log to exact offsets, and only those are downloaded.  Only when
     * the arena itself runs out (or a log outgrows its second extent) is the replay launched again, with exact capacities. */
    std::vector<uint64_t> xoff((size_t)L + 1, 0);
    /* (tests: PTX_REPLAY_NO_ARENA=1 plays a device too full for the arena, PTX_REPLAY_PACK_RECORDS=<n> one too full for the packed copy) */
    const bool no_arena_env = getenv("PTX_REPLAY_NO_ARENA") != nullptr;
    const uint64_t pack_env = getenv("PTX_REPLAY_PACK_RECORDS") ? (uint64_t)std::max<long long>(atoll(getenv("PTX_REPLAY_PACK_RECORDS")), 1) : 0;
    for (uint32_t attempt = 0; attempt < 2 && st == PTX_OK; ++attempt) {
        const uint64_t total = h->off[L];
        uint64_t arena_cap = attempt == 0 && !no_arena_env ? total + 65536 : 0;
        e = ptx_dev_malloc((void**)&d_off, ((size_t)L + 1) * 8);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_ext, (size_t)L * 24);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_xoff, ((size_t)L + 1) * 8);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_next, 8);
        if (e == hipSuccess) e = ptx_dev_malloc((void**)&d_logs, (size_t)L * sizeof(ptx_patch_log));
        if (e == hipSuccess) {
            e = ptx_dev_malloc((void**)&d_patches, std::max<uint64_t>(total + arena_cap, 1) * sizeof(ptx_patch));
            if (e == hipErrorOutOfMemory && arena_cap) { /* no room for the arena: the capacities alone (a log that outgrows its own is then replayed again with exact sizes) */
                (void)hipGetLastError();
                arena_cap = 0;
                e = ptx_dev_malloc((void**)&d_patches, std::max<uint64_t>(total, 1) * sizeof(ptx_patch));
            }
        }
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, h->off.data(), ((size_t)L + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_next, 0, 8, ctx->stream);
        if (e == hipSuccess) {
            PtxReplayArgs A;
            A.log_off = b->log_off;
            A.op_id = b->op_id;
            A.ref_a = b->ref_a;
            A.ref_b = b->ref_b;
            A.payload = b->payload;
            A.action = b->action;
            A.mark_type = b->mark_type;
            A.side_a = b->side_a;
            A.side_b = b->side_b;
            A.log_hdr = b->log_hdr;
            A.res = r->logs;
            A.elem_rank = r->rank;
            A.refs = r->refs;
            A.refs_hi = r->refs_hi;
            A.patch_off = d_off;
            A.patches = d_patches;
            A.plogs = d_logs;
            A.n_logs = L;
            A.lds_bytes = lds_bytes;
            A.win_scratch = d_win;
            A.win_off = d_winoff;
            A.first_row = d_first;
            A.arena_next = arena_cap ? d_next : nullptr;
            A.arena_base = total;
            A.arena_cap = arena_cap;
            A.ext_off = d_ext;
            (void)hipEventRecord(ctx->ev0, ctx->stream);
            if (!n_lds) { /* (every log belongs to the launch below) */
            } else if (wide) hipLaunchKernelGGL(ptx_replay_kernel_wide, dim3(L), dim3(PTX_REPLAY_THREADS), lds_bytes, ctx->stream, A);
            else if (gwin) hipLaunchKernelGGL(ptx_replay_kernel_gwin, dim3(L), dim3(PTX_REPLAY_THREADS), lds_bytes, ctx->stream, A);
            else hipLaunchKernelGGL(ptx_replay_kernel, dim3(L), dim3(PTX_REPLAY_THREADS), lds_bytes, ctx->stream, A);
            e = hipGetLastError();
            if (e == hipSuccess && n_hbm) { /* behind it on the stream: the same records / plogs / extents / arena, the logs of hbm_logs */
                PtxReplayHbmArgs HA;
                HA.R = A;
                HA.state = d_state;
                HA.state_off = d_soff;
                HA.log_index = d_hidx;
                HA.n_hbm = n_hbm;
                hipLaunchKernelGGL(ptx_replay_kernel_hbm, dim3(n_hbm), dim3(PTX_REPLAY_THREADS), 0, ctx->stream, HA);
                e = hipGetLastError();
            }
            (void)hipEventRecord(ctx->ev1, ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h->logs.data(), d_logs, (size_t)L * sizeof(ptx_patch_log), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) (void)hipEventElapsedTime(&out->kernel_ms, ctx->ev0, ctx->ev1);
        if (e != hipSuccess) {
            st = fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_replay_kernel: ") + hipGetErrorString(e));
            break;
        }
        out->launches = attempt + 1;
        bool over = false; /* a log that produced records and reports PTX_ERR_CAPACITY ran out of room for them (one whose working set exceeds the LDS produces none) */
        for (uint32_t l = 0; l < L; ++l) over = over || (h->logs[l].status == PTX_ERR_CAPACITY && h->logs[l].n_patches != 0);
        if (!over || attempt == 1) {
            for (uint32_t l = 0; l < L; ++l) xoff[l + 1] = xoff[l] + (h->logs[l].status == PTX_OK ? h->logs[l].n_patches : 0u);
            const uint64_t xtotal = xoff[L];
            /* the packed copy: the whole stream at once — or, where device memory is short, as large a buffer as there is (never smaller than the longest log's
             * stream), filled and downloaded a range of logs at a time */
            uint64_t longest = 1, pack_cap = std::max<uint64_t>(xtotal, 1);
            for (uint32_t l = 0; l < L; ++l) longest = std::max<uint64_t>(longest, xoff[l + 1] - xoff[l]);
            if (pack_env) pack_cap = std::max<uint64_t>(std::min<uint64_t>(pack_cap, pack_env), longest);
            for (;;) {
                e = ptx_dev_malloc((void**)&d_packed, pack_cap * sizeof(ptx_patch));
                if (e != hipErrorOutOfMemory || pack_cap == longest) break;
                (void)hipGetLastError();
                pack_cap = std::max<uint64_t>(pack_cap / 2, longest);
            }
            if (e == hipSuccess) e = hipMemcpyAsync(d_xoff, xoff.data(), ((size_t)L + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
            h->patches.resize(sink ? 1 : std::max<uint64_t>(xtotal, 1));
            PtxAccumScratch scratch;
            if (sink && e == hipSuccess) { /* the accumulate launches' blocks, once, for the largest of the ranges below */
                uint64_t most_logs = 0, most_units = 0;
                for (uint32_t l0 = 0; l0 < L;) {
                    uint32_t l1 = l0 + 1;
                    while (l1 < L && xoff[l1 + 1] - xoff[l0] <= pack_cap) ++l1;
                    most_logs = std::max<uint64_t>(most_logs, l1 - l0);
                    most_units = std::max(most_units, accum_range_state_units(ctx, hdr, log_off, l0, l1));
                    l0 = l1;
                }
                e = accum_scratch_reserve(&scratch, most_logs, most_units);
            }
            for (uint32_t l0 = 0; e == hipSuccess && l0 < L;) {
                uint32_t l1 = l0 + 1;
                while (l1 < L && xoff[l1 + 1] - xoff[l0] <= pack_cap) ++l1;
                const uint64_t cnt = xoff[l1] - xoff[l0];
                if (sink) { /* the range is accumulated where it sits (a log without records has a row of its own too) */
                    if (cnt) {
                        hipLaunchKernelGGL(ptx_patch_pack_kernel, dim3(l1 - l0), dim3(256), 0, ctx->stream, d_patches, d_off, d_ext, d_xoff, d_packed, l0, xoff[l0]);
                        e = hipGetLastError();
                    }
                    if (e == hipSuccess) {
                        PtxAccumArgs AA;
                        memset(&AA, 0, sizeof(AA));
                        AA.log_off = b->log_off;
                        AA.payload = b->payload;
                        AA.action = b->action;
                        AA.mark_type = b->mark_type;
                        AA.log_hdr = b->log_hdr;
                        AA.patches = d_packed;
                        AA.rec_off = d_xoff;
                        AA.rec_base = xoff[l0];
                        AA.plogs = d_logs;
                        AA.want = sink->want->logs;
                        AA.check = sink->d_check;
                        st = accum_launch_range(ctx, &scratch, hdr, log_off, l0, l1, AA, &sink->accum_ms); /* (waits: the buffer is filled again) */
                        if (st != PTX_OK) break;
                    }
                } else if (cnt) {
                    hipLaunchKernelGGL(ptx_patch_pack_kernel, dim3(l1 - l0), dim3(256), 0, ctx->stream, d_patches, d_off, d_ext, d_xoff, d_packed, l0, xoff[l0]);
                    e = hipGetLastError();
                    if (e == hipSuccess) e = hipMemcpyAsync(h->patches.data() + xoff[l0], d_packed, cnt * sizeof(ptx_patch), hipMemcpyDeviceToHost, ctx->stream);
                    if (e == hipSuccess && l1 < L) e = hipStreamSynchronize(ctx->stream); /* the buffer is filled again */
                }
                l0 = l1;
            }
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            accum_scratch_free(&scratch);
            if (e != hipSuccess && st == PTX_OK) st = fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("patch download: ") + hipGetErrorString(e));
            h->off = xoff;
            break;
        }
        /* the arena ran out, or a log outgrew its extent: exact capacities, once more */
        for (uint32_t l = 0; l < L; ++l) h->off[l + 1] = h->off[l] + std::max<uint64_t>(h->logs[l].n_patches, 1);
        release();
    }
    release();
    release_setup();
    if (st != PTX_OK) {
        ptx_patches_free(out);
        return st;
    }
    out->patch_off = h->off.data();
    out->logs = h->logs.data();
    out->patches = h->patches.data();
    return PTX_OK;
}

/* ---- patch streams back into canonical rows (accum_core.h) ---- */
ptx_status ptx_accumulate_patches(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_patches* p, ptx_result* out) {
    if (!ctx || !b || !p || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    const uint32_t L = b->n_logs;
    if (p->n_logs != L) return fail(ctx, PTX_ERR_INVALID_ARG, "the patch streams do not match the batch");
    if (L && (!p->patch_off || !p->logs)) return fail(ctx, PTX_ERR_INVALID_ARG, "patch_off / logs missing");
    const uint64_t total = L ? p->patch_off[L] : 0;
    for (uint32_t l = 0; l < L; ++l)
        if (p->logs[l].status == PTX_OK && (p->patch_off[l] > total || p->logs[l].n_patches > total - p->patch_off[l]))
            return fail(ctx, PTX_ERR_INVALID_ARG, "a log's records run past patch_off[n_logs]");
    if (total && !p->patches) return fail(ctx, PTX_ERR_INVALID_ARG, "patches missing");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dresult tmp; /* rows where the merge's go; no elem_rank */
    tmp.n_logs = L;
    tmp.n_rows = b->n_ops;
    std::vector<ptx_log_hdr> hdr(L);
    std::vector<uint64_t> log_off((size_t)L + 1, 0);
    ptx_patch* d_pat = nullptr;
    uint64_t* d_poff = nullptr;
    ptx_patch_log* d_plogs = nullptr;
    hipError_t e = dalloc(&tmp.logs, L);
    if (e == hipSuccess) e = dalloc(&tmp.values, tmp.n_rows);
    if (e == hipSuccess) e = dalloc(&tmp.spans, tmp.n_rows);
    if (e == hipSuccess) e = dalloc(&tmp.cints, tmp.n_rows);
    if (e == hipSuccess) e = dalloc(&d_pat, total);
    if (e == hipSuccess) e = dalloc(&d_poff, (uint64_t)L + 1);
    if (e == hipSuccess) e = dalloc(&d_plogs, L);
    if (e == hipSuccess && L) e = hipMemcpyAsync(hdr.data(), b->log_hdr, (size_t)L * sizeof(ptx_log_hdr), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && L) e = hipMemcpyAsync(log_off.data(), b->log_off, ((size_t)L + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && total) e = hipMemcpyAsync(d_pat, p->patches, total * sizeof(ptx_patch), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && L) e = hipMemcpyAsync(d_poff, p->patch_off, ((size_t)L + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && L) e = hipMemcpyAsync(d_plogs, p->logs, (size_t)L * sizeof(ptx_patch_log), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    ptx_status st = e == hipSuccess ? PTX_OK : fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_accumulate_patches set-up: ") + hipGetErrorString(e));
    if (st == PTX_OK && L) {
        PtxAccumArgs A;
        memset(&A, 0, sizeof(A));
        A.log_off = b->log_off;
        A.payload = b->payload;
        A.action = b->action;
        A.mark_type = b->mark_type;
        A.log_hdr = b->log_hdr;
        A.patches = d_pat;
        A.rec_off = d_poff;
        A.rec_base = 0;
        A.plogs = d_plogs;
        A.res = tmp.logs;
        A.out_values = tmp.values;
        A.out_spans = tmp.spans;
        A.out_cints = tmp.cints;
        PtxAccumScratch scratch;
        st = accum_launch_range(ctx, &scratch, hdr, log_off, 0, L, A, nullptr);
        accum_scratch_free(&scratch);
    }
    if (st == PTX_OK) st = ptx_result_download(ctx, b, &tmp, out);
    (void)ptx_dev_free(tmp.logs);
    (void)ptx_dev_free(tmp.values);
    (void)ptx_dev_free(tmp.spans);
    (void)ptx_dev_free(tmp.cints);
    (void)ptx_dev_free(d_pat);
    (void)ptx_dev_free(d_poff);
    (void)ptx_dev_free(d_plogs);
    return st;
}

ptx_status ptx_check_patches(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, ptx_patch_check_log* out, uint64_t* n_disagree) {
    if (!ctx || !b || !r || !out || !n_disagree) return PTX_ERR_INVALID_ARG;
    *n_disagree = 0;
    const uint32_t L = b->n_logs;
    if (r->n_logs != L || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "result buffers do not match the batch");
    if (!r->rank) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_check_patches needs the elem_rank column (context created with PTX_FLAG_NO_ELEM_RANK)");
    if (L == 0) return PTX_OK;
    PTX_HIP(ctx, ptx_enter(ctx));
    PtxAccumSink sink;
    sink.want = r;
    sink.d_check = nullptr;
    sink.accum_ms = 0.f;
    PTX_HIP(ctx, dalloc(&sink.d_check, L));
    ptx_patches pat;
    ptx_status st = replay_patches_impl(ctx, b, r, nullptr, &pat, &sink);
    if (st == PTX_OK) {
        ctx->check_replay_ms = pat.kernel_ms;
        ctx->check_accum_ms = sink.accum_ms;
        ptx_patches_free(&pat);
        /* the one download of the answer: 32 bytes per log */
        hipError_t e = hipMemcpyAsync(out, sink.d_check, (size_t)L * sizeof(ptx_patch_check_log), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) st = fail(ctx, PTX_ERR_HIP, std::string("ptx_check_patches download: ") + hipGetErrorString(e));
    }
    (void)ptx_dev_free(sink.d_check);
    if (st == PTX_OK)
        for (uint32_t l = 0; l < L; ++l) *n_disagree += out[l].status == PTX_OK && out[l].agrees == 0u ? 1u : 0u;
    return st;
}

ptx_status ptx_check_patches_ms(const ptx_ctx* ctx, float* replay_ms, float* accum_ms) {
    if (!ctx || !replay_ms || !accum_ms) return PTX_ERR_INVALID_ARG;
    *replay_ms = ctx->check_replay_ms;
    *accum_ms = ctx->check_accum_ms;
    return PTX_OK;
}

/* ---- on-device change() ---- */
struct ptx_host_gen {
    std::vector<uint32_t> n_comments;
};
void ptx_gen_info_free(ptx_gen_info* info) {
    if (!info) return;
    delete (ptx_host_gen*)info->owner;
    memset(info, 0, sizeof(*info));
}

ptx_status ptx_generate(ptx_ctx* ctx, const ptx_gen_config* cfg, ptx_dbatch** out, ptx_gen_info* info) {
    if (!ctx || !cfg || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    if (info) memset(info, 0, sizeof(*info));
    if (cfg->replicas < 1 || cfg->replicas > PTX_GEN_MAX_R || cfg->n_mark_types > 4 || cfg->ops_per_log < 1 || cfg->ops_per_log > 65533u ||
        cfg->mix[0] > 100u || cfg->mix[1] > 100u || cfg->mix[2] > 100u || cfg->mix[3] > 100u || cfg->mix[0] + cfg->mix[1] + cfg->mix[2] + cfg->mix[3] != 100u)
        return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_generate: 1..8 replicas, at most 65533 ops per log, mix percentages summing to 100");
    for (uint32_t i = 0; i < cfg->n_mark_types; ++i)
        if (cfg->mark_types[i] > PTX_MARK_LINK) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_generate: mark_types must be PTX_MARK_* values");
    const size_t tl = strnlen(cfg->initial_text, sizeof(cfg->initial_text));
    const char* text = tl ? cfg->initial_text : "ABCDE";
    const uint32_t init_len = (uint32_t)(tl ? tl : 5);
    if (init_len > cfg->ops_per_log || tl >= sizeof(cfg->initial_text)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_generate: initial text too long");
    PTX_HIP(ctx, ptx_enter(ctx));
    const uint32_t R = cfg->replicas, N = cfg->ops_per_log + 1u, D = cfg->n_docs;
    if ((uint64_t)D * R > 0xFFFFFFFFull) return fail(ctx, PTX_ERR_INVALID_ARG, "too many logs");
    ptx_dbatch* b = new ptx_dbatch();
    b->n_logs = D * R;
    b->n_ops = (uint64_t)b->n_logs * N;
    b->max_actors = R;
    const uint64_t T = b->n_ops;
    uint32_t *cap_hdr = nullptr, *d_nchg = nullptr, *d_ncom = nullptr, *d_status = nullptr;
    uint16_t* cap_env = nullptr;
    uint8_t* d_ctab = nullptr; /* PtxGenChangeT<ptx_gen_max_r(R)> per op */
    uint16_t* d_known = nullptr;
    auto drop = [&]() { /* idempotent: a later failure path may call it again */
        (void)ptx_dev_free(cap_hdr);
        (void)ptx_dev_free(cap_env);
        (void)ptx_dev_free(d_nchg);
        (void)ptx_dev_free(d_ncom);
        (void)ptx_dev_free(d_status);
        (void)ptx_dev_free(d_ctab);
        (void)ptx_dev_free(d_known);
        cap_hdr = d_nchg = d_ncom = d_status = nullptr;
        cap_env = nullptr;
        d_ctab = nullptr;
        d_known = nullptr;
    };
#define PTX_TRYG(call)                                  \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string m = std::string(#call) + ": " + hipGetErrorString(_e); \
            drop();                                     \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, m); \
        }                                               \
    } while (0)
    PTX_TRYG(dalloc(&b->log_off, (uint64_t)b->n_logs + 1));
    PTX_TRYG(dalloc(&b->op_id, T));
    PTX_TRYG(dalloc(&b->ref_a, T));
    PTX_TRYG(dalloc(&b->ref_b, T));
    PTX_TRYG(dalloc(&b->payload, T));
    PTX_TRYG(dalloc(&b->action, T + PTX_BYTE_PAD));
    PTX_TRYG(dalloc(&b->mark_type, T + PTX_BYTE_PAD));
    PTX_TRYG(dalloc(&b->side_a, T));
    PTX_TRYG(dalloc(&b->side_b, T));
    PTX_TRYG(dalloc(&b->log_hdr, (uint64_t)b->n_logs));
    PTX_TRYG(dalloc(&b->chg_off, (uint64_t)b->n_logs + 1));
    PTX_TRYG(dalloc(&cap_hdr, T));
    PTX_TRYG(dalloc(&cap_env, T * PTX_ENV_STRIDE(R)));
    PTX_TRYG(dalloc(&d_nchg, (uint64_t)b->n_logs));
    PTX_TRYG(dalloc(&d_ncom, (uint64_t)D));
    PTX_TRYG(dalloc(&d_status, (uint64_t)D));
    PTX_TRYG(dalloc(&d_ctab, T * ptx_gen_change_bytes(R)));
    PTX_TRYG(dalloc(&d_known, T));
    if (D == 0) {
        drop();
        PTX_TRYG(hipMemsetAsync(b->log_off, 0, 8, ctx->stream));
        PTX_TRYG(hipMemsetAsync(b->chg_off, 0, 8, ctx->stream));
        PTX_TRYG(hipStreamSynchronize(ctx->stream));
        shape_launch(ctx, b, 0, 0);
        *out = b;
        return PTX_OK;
    }
    PtxGenArgs A;
    memset(&A, 0, sizeof(A));
    A.n_docs = D;
    A.first_doc = cfg->first_doc;
    A.seed = cfg->seed;
    A.R = R;
    A.ops_per_log = cfg->ops_per_log;
    A.mix0 = cfg->mix[0];
    A.mix01 = cfg->mix[0] + cfg->mix[1];
    A.mix012 = cfg->mix[0] + cfg->mix[1] + cfg->mix[2];
    A.n_mark_types = cfg->n_mark_types;
    memcpy(A.mark_types, cfg->mark_types, 4);
    A.init_len = init_len;
    memcpy(A.init_text, text, init_len);
    A.rows_per_log = N;
    A.list_cap = cfg->list_cap ? cfg->list_cap : N + 8u;
    const uint64_t need = ptx_gen_lds_need(R, A.list_cap, N);
    if (need > ctx->max_lds) {
        drop();
        ptx_batch_free(ctx, b);
        return fail(ctx, PTX_ERR_CAPACITY, "ptx_generate: list_cap x replicas exceeds the LDS of a CU; pass a smaller list_cap");
    }
    A.lds_bytes = (uint32_t)((need + 255) & ~255ull);
    A.op_id = b->op_id;
    A.ref_a = b->ref_a;
    A.ref_b = b->ref_b;
    A.payload = b->payload;
    A.action = b->action;
    A.mark_type = b->mark_type;
    A.side_a = b->side_a;
    A.side_b = b->side_b;
    A.chg_hdr = cap_hdr;
    A.chg_env = cap_env;
    A.n_changes = d_nchg;
    A.n_comments = d_ncom;
    A.status = d_status;
    A.ctab = d_ctab;
    A.known = d_known;
    hipLaunchKernelGGL(ptx_regular_offsets_kernel, dim3((b->n_logs + 256) / 256), dim3(256), 0, ctx->stream, b->log_off, b->n_logs, (uint64_t)N);
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    if (R <= 4) hipLaunchKernelGGL(ptx_gen_kernel, dim3(D), dim3(64), A.lds_bytes, ctx->stream, A);
    else hipLaunchKernelGGL(ptx_gen_kernel_r8, dim3(D), dim3(64), A.lds_bytes, ctx->stream, A);
    PTX_TRYG(hipGetLastError());
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    std::vector<uint32_t> nchg(b->n_logs), status(D);
    ptx_host_gen* hg = new ptx_host_gen();
    hg->n_comments.resize(D);
    hipError_t e = hipMemcpyAsync(nchg.data(), d_nchg, (size_t)b->n_logs * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(status.data(), d_status, (size_t)D * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hg->n_comments.data(), d_ncom, (size_t)D * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    float ms = 0;
    if (e == hipSuccess) (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    uint32_t failed = 0;
    for (uint32_t d = 0; d < D && e == hipSuccess; ++d) failed += status[d] != PTX_OK;
    if (e != hipSuccess || failed) {
        delete hg;
        drop();
        ptx_batch_free(ctx, b);
        if (e != hipSuccess) return fail(ctx, PTX_ERR_HIP, std::string("ptx_gen_kernel: ") + hipGetErrorString(e));
        return fail(ctx, PTX_ERR_CAPACITY, std::to_string(failed) + " generated document(s) outgrew list_cap");
    }
    /* compact the envelope */
    std::vector<uint64_t> coff((size_t)b->n_logs + 1, 0);
    for (uint32_t l = 0; l < b->n_logs; ++l) coff[l + 1] = coff[l] + nchg[l];
    const uint64_t NC = coff[b->n_logs];
    b->n_changes = NC;
    auto fin = [&](hipError_t err) { /* error after this point */
        delete hg;
        drop();
        ptx_batch_free(ctx, b);
        return fail(ctx, err == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_generate: ") + hipGetErrorString(err));
    };
    e = dalloc(&b->chg_hdr, NC + PTX_ENV_PAD);
    if (e == hipSuccess) e = dalloc(&b->chg_env, (NC + PTX_ENV_PAD) * PTX_ENV_STRIDE(R));
    if (e == hipSuccess) e = hipMemcpyAsync(b->chg_off, coff.data(), ((size_t)b->n_logs + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fin(e);
    hipLaunchKernelGGL(ptx_gen_compact_kernel, dim3(b->n_logs), dim3(256), 0, ctx->stream, b->chg_off, N, R, cap_hdr, cap_env, b->chg_hdr, b->chg_env);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fin(e);
    drop();
    const ptx_status st = census_and_shape(ctx, b, false);
    if (st != PTX_OK) {
        delete hg;
        ptx_batch_free(ctx, b);
        return st;
    }
    if (info) {
        info->n_docs = D;
        info->kernel_ms = ms;
        info->n_comments = hg->n_comments.data();
        info->owner = hg;
    } else {
        delete hg;
    }
    *out = b;
    return PTX_OK;
#undef PTX_TRYG
}

/* ---- the map objects of a replica: getRoot() ---- */
struct ptx_host_root_maps {
    std::vector<uint64_t> off;
    std::vector<ptx_root_log> logs;
    std::vector<ptx_root_entry> entries;
};
void ptx_root_maps_free(ptx_root_maps* m) {
    if (!m) return;
    delete (ptx_host_root_maps*)m->owner;
    memset(m, 0, sizeof(*m));
}
ptx_status ptx_root_map(ptx_ctx* ctx, const ptx_dbatch* b, ptx_root_maps* out) {
    if (!ctx || !b || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_root_maps* h = new ptx_host_root_maps();
    const uint32_t L = b->n_logs;
    h->off.assign((size_t)L + 1, 0);
    h->logs.resize(std::max<uint32_t>(L, 1));
    h->entries.resize(1);
    out->owner = h;
    out->n_logs = L;
    out->entry_off = h->off.data();
    out->logs = h->logs.data();
    out->entries = h->entries.data();
    if (L == 0) return PTX_OK;
    uint32_t* d_cnt = nullptr;
    uint64_t* d_off = nullptr;
    ptx_root_log* d_logs = nullptr;
    ptx_root_entry* d_ent = nullptr;
    auto release = [&]() {
        (void)ptx_dev_free(d_cnt);
        (void)ptx_dev_free(d_off);
        (void)ptx_dev_free(d_logs);
        (void)ptx_dev_free(d_ent);
    };
    std::vector<uint32_t> cnt(L);
    hipError_t e = dalloc(&d_cnt, L);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ptx_rootmap_count_kernel, dim3(L), dim3(64), 0, ctx->stream, b->log_off, b->action, L, d_cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)L * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    uint32_t most = 0;
    if (e == hipSuccess) {
        for (uint32_t l = 0; l < L; ++l) {
            h->off[l + 1] = h->off[l] + cnt[l];
            most = std::max(most, cnt[l]);
        }
        const uint64_t total = h->off[L];
        h->entries.resize(std::max<uint64_t>(total, 1));
        out->entries = h->entries.data();
        e = dalloc(&d_off, (uint64_t)L + 1);
        if (e == hipSuccess) e = dalloc(&d_logs, L);
        if (e == hipSuccess) e = dalloc(&d_ent, std::max<uint64_t>(total, 1));
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, h->off.data(), ((size_t)L + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) {
        PtxRootArgs A;
        A.log_off = b->log_off;
        A.op_id = b->op_id;
        A.ref_a = b->ref_a;
        A.ref_b = b->ref_b;
        A.payload = b->payload;
        A.action = b->action;
        A.mark_type = b->mark_type;
        A.entry_off = d_off;
        A.entries = d_ent;
        A.rlogs = d_logs;
        A.n_logs = L;
        /* logs with more map ops than the LDS of a CU holds report PTX_ERR_CAPACITY */
        A.lds_bytes = (uint32_t)std::min<uint64_t>((ptx_rootmap_lds_need(most) + 255) & ~255ull, ctx->max_lds);
        hipLaunchKernelGGL(ptx_rootmap_kernel, dim3(L), dim3(64), A.lds_bytes, ctx->stream, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h->logs.data(), d_logs, (size_t)L * sizeof(ptx_root_log), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h->off[L]) e = hipMemcpyAsync(h->entries.data(), d_ent, (size_t)h->off[L] * sizeof(ptx_root_entry), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    release();
    if (e != hipSuccess) {
        ptx_root_maps_free(out);
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_root_map: ") + hipGetErrorString(e));
    }
    return PTX_OK;
}

/* ---- cursors ---- */
ptx_status ptx_resolve_cursors(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, uint32_t n_queries, const uint32_t* q_log, const uint8_t* q_kind,
                               const uint64_t* q_arg, uint64_t* out, uint32_t* status_out) {
    if (!ctx || !b || !r || (n_queries && (!q_log || !q_kind || !q_arg || !out || !status_out))) return PTX_ERR_INVALID_ARG;
    if (r->n_logs != b->n_logs || r->n_rows != b->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_resolve_cursors: `r` is not the result of this batch");
    if (!r->rank) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_resolve_cursors needs the elem_rank column (context created with PTX_FLAG_NO_ELEM_RANK)");
    if (n_queries == 0) return PTX_OK;
    for (uint32_t q = 0; q < n_queries; ++q)
        if (q_log[q] >= b->n_logs || q_kind[q] > PTX_CURSOR_GET) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_resolve_cursors: a query names no log of the batch or an unknown kind");
    PTX_HIP(ctx, ptx_enter(ctx));
    /* group the queries by log: one workgroup builds a log's index once and answers all of them */
    std::vector<uint32_t> perm(n_queries);
    for (uint32_t q = 0; q < n_queries; ++q) perm[q] = q;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return q_log[x] < q_log[y]; });
    std::vector<uint32_t> glog;
    std::vector<uint64_t> goff;
    for (uint32_t k = 0; k < n_queries; ++k)
        if (k == 0 || q_log[perm[k]] != q_log[perm[k - 1]]) {
            glog.push_back(q_log[perm[k]]);
            goff.push_back(k);
        }
    goff.push_back(n_queries);
    const uint32_t G = (uint32_t)glog.size();
    std::vector<ptx_log_hdr> hdr(b->n_logs);
    PTX_HIP(ctx, hipMemcpyAsync(hdr.data(), b->log_hdr, (size_t)b->n_logs * sizeof(ptx_log_hdr), hipMemcpyDeviceToHost, ctx->stream));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> loff((size_t)b->n_logs + 1);
    PTX_HIP(ctx, hipMemcpyAsync(loff.data(), b->log_off, ((size_t)b->n_logs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t need = 4096;
    for (uint32_t l : glog) {
        /* the indexed form where the log fits it (16-bit row indices, one CU's LDS), else the long-document form (cursor_core.h): the kernel takes the same decision */
        const uint64_t ks = ((uint64_t)hdr[l].max_counter + 1) * ((uint64_t)hdr[l].max_actor + 1);
        const bool indexed = ptx_cursor_indexed(loff[l + 1] - loff[l], hdr[l].n_ins, hdr[l].max_actor, ks, ctx->max_lds);
        need = std::max<uint64_t>(need, indexed ? ptx_cursor_lds_need(hdr[l].n_ins, ks) : ptx_cursor_lds_need_long(hdr[l].n_ins));
    }
    const uint32_t lds_bytes = (uint32_t)std::min<uint64_t>((need + 255) & ~255ull, ctx->max_lds); /* (documents of more than ~600 000 elements report PTX_ERR_CAPACITY) */
    uint32_t *d_glog = nullptr, *d_perm = nullptr, *d_status = nullptr;
    uint64_t *d_goff = nullptr, *d_arg = nullptr, *d_out = nullptr;
    uint8_t* d_kind = nullptr;
    auto drop = [&]() {
        for (void* p : {(void*)d_glog, (void*)d_perm, (void*)d_status, (void*)d_goff, (void*)d_arg, (void*)d_out, (void*)d_kind}) (void)ptx_dev_free(p);
    };
    hipError_t e = dalloc(&d_glog, G);
    if (e == hipSuccess) e = dalloc(&d_goff, (uint64_t)G + 1);
    if (e == hipSuccess) e = dalloc(&d_perm, n_queries);
    if (e == hipSuccess) e = dalloc(&d_kind, n_queries);
    if (e == hipSuccess) e = dalloc(&d_arg, n_queries);
    if (e == hipSuccess) e = dalloc(&d_out, n_queries);
    if (e == hipSuccess) e = dalloc(&d_status, n_queries);
    if (e == hipSuccess) e = hipMemcpyAsync(d_glog, glog.data(), (size_t)G * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_goff, goff.data(), ((size_t)G + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_perm, perm.data(), (size_t)n_queries * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_kind, q_kind, (size_t)n_queries, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_arg, q_arg, (size_t)n_queries * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        PtxCursorArgs A;
        memset(&A, 0, sizeof(A));
        A.log_off = b->log_off;
        A.op_id = b->op_id;
        A.action = b->action;
        A.log_hdr = b->log_hdr;
        A.res = r->logs;
        A.elem_rank = r->rank;
        A.q_group_log = d_glog;
        A.q_group_off = d_goff;
        A.q_perm = d_perm;
        A.q_kind = d_kind;
        A.q_arg = d_arg;
        A.out = d_out;
        A.status = d_status;
        A.n_groups = G;
        A.lds_bytes = lds_bytes;
        hipLaunchKernelGGL(ptx_cursor_kernel, dim3(G), dim3(PTX_CURSOR_THREADS), lds_bytes, ctx->stream, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n_queries * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(status_out, d_status, (size_t)n_queries * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    drop();
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_resolve_cursors: ") + hipGetErrorString(e));
    return PTX_OK;
}

/* ---- change(): caller-supplied InputOperations ---- */
ptx_status ptx_change(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_dresult* merged, const ptx_input_ops* in, ptx_dbatch** made, uint32_t* status_out) {
    if (!ctx || !base || !merged || !in || !made || !status_out) return PTX_ERR_INVALID_ARG;
    *made = nullptr;
    const uint32_t L = base->n_logs;
    if (in->n_logs != L) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: the InputOperations must name every log of the base batch (a log may make no change)");
    if (merged->n_logs != L || merged->n_rows != base->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: `merged` is not the result of this batch");
    if (!merged->rank) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change needs the elem_rank column (context created with PTX_FLAG_NO_ELEM_RANK)");
    if (L && (!in->chg_off || !in->op_off || !in->actor)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: chg_off / op_off / actor is NULL");
    if (base->n_ops && !base->chg_off) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change needs the Change envelope of the base batch (the replicas' clocks)");
    const uint32_t na = base->chg_off && base->n_changes ? base->max_actors : in->max_actors;
    if (na == 0 || na > 4096u || (base->chg_off && base->n_changes && in->max_actors && in->max_actors != base->max_actors))
        return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: max_actors must be 1..4096 and equal to the base batch's");
    const uint64_t NC = L ? in->chg_off[L] : 0;
    const uint64_t NI = NC ? in->op_off[NC] : 0;
    if (L && in->chg_off[0] != 0) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: chg_off must start at 0");
    for (uint32_t l = 0; l < L; ++l)
        if (in->chg_off[l + 1] < in->chg_off[l]) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: chg_off decreases");
    if (NC && in->op_off[0] != 0) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: op_off must start at 0");
    for (uint64_t c = 0; c < NC; ++c)
        if (in->op_off[c + 1] < in->op_off[c]) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: op_off decreases");
    if (NI && (!in->action || !in->mark_type || !in->index || !in->count || !in->payload)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: an InputOperation column is NULL");
    /* rows every log will make (known up front: one per inserted value, per deleted element, per mark, per makeList) */
    std::vector<uint64_t> out_off((size_t)L + 1, 0);
    std::vector<uint32_t> grow(L, 0);
    for (uint32_t l = 0; l < L; ++l) {
        uint64_t rows = 0;
        for (uint64_t q = in->op_off[in->chg_off[l]]; q < in->op_off[in->chg_off[l + 1]]; ++q) {
            const uint8_t a = in->action[q];
            if (a == PTX_IN_INSERT) {
                if ((uint64_t)in->payload[q] + in->count[q] > in->n_values || (in->count[q] && !in->values)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: an insert points outside `values`");
                rows += in->count[q];
                grow[l] += in->count[q];
            } else if (a == PTX_IN_DELETE) rows += in->count[q];
            else rows += 1;
            if (rows > PTX_CHANGE_ROWS_MAX) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: more than 65534 ops for one log");
        }
        out_off[l + 1] = out_off[l] + rows;
    }
    const uint64_t T = out_off[L];
    PTX_HIP(ctx, ptx_enter(ctx));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    /* launch shape: the LDS of the largest working set among the logs that make a change */
    std::vector<ptx_log_hdr> hdr(std::max<uint32_t>(L, 1));
    std::vector<uint64_t> log_off((size_t)L + 1, 0);
    if (L) {
        PTX_HIP(ctx, hipMemcpyAsync(hdr.data(), base->log_hdr, (size_t)L * sizeof(ptx_log_hdr), hipMemcpyDeviceToHost, ctx->stream));
        PTX_HIP(ctx, hipMemcpyAsync(log_off.data(), base->log_off, ((size_t)L + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    uint64_t need = 4096;
    /* round 6: the element list of a log that does not fit one CU's LDS (more than ~40 000 elements) lives in a slice of global scratch */
    /* (tests: PTX_CHANGE_LIST_IN_HBM=1 puts the list of EVERY log there, so that documents of a few dozen elements run the form) */
    const bool all_in_hbm = getenv("PTX_CHANGE_LIST_IN_HBM") != nullptr;
    std::vector<uint64_t> list_off((size_t)L + 1, 0);
    for (uint32_t l = 0; l < L; ++l) {
        list_off[l + 1] = list_off[l];
        if (in->chg_off[l + 1] > in->chg_off[l]) {
            const bool rows = log_off[l + 1] > log_off[l];
            const uint64_t ks = rows ? ((uint64_t)hdr[l].max_counter + 1) * ((uint64_t)std::min<uint32_t>(hdr[l].max_actor, 4095u) + 1) : 1;
            const uint64_t n_l = rows ? hdr[l].n_ins : 0;
            const bool in_hbm = all_in_hbm || ptx_change_lds_need(n_l, grow[l], ks, na) > ctx->max_lds;
            if (in_hbm) list_off[l + 1] += ptx_change_list_words(n_l, grow[l]);
            need = std::max<uint64_t>(need, ptx_change_lds_need(n_l, grow[l], ks, na, in_hbm));
        }
    }
    const uint32_t lds_bytes = (uint32_t)std::min<uint64_t>((need + 255) & ~255ull, ctx->max_lds); /* larger logs report PTX_ERR_CAPACITY */

    ptx_dbatch* cap = new ptx_dbatch(); /* the kernel's capacity-layout output, owned here */
    ptx_dbatch* b = nullptr;
    uint64_t *d_in_chg = nullptr, *d_in_op = nullptr, *d_out_off = nullptr, *d_doff = nullptr, *d_dcoff = nullptr;
    uint8_t *d_in_action = nullptr, *d_in_mt = nullptr;
    uint32_t *d_in_index = nullptr, *d_in_count = nullptr, *d_in_payload = nullptr, *d_in_values = nullptr, *d_actor = nullptr, *d_status = nullptr, *d_rows = nullptr, *d_chgs = nullptr;
    uint32_t* d_list = nullptr;
    uint64_t* d_list_off = nullptr;
    uint8_t* d_pack = nullptr; /* the small inputs of the call as ONE block, uploaded with one copy (the d_in_* pointers then point into it) */
    uint32_t* d_outw = nullptr; /* status / rows made / changes made per log + the "some high half is set" word: one block, one copy back */
    auto drop = [&]() {
        ptx_batch_free(ctx, cap);
        cap = nullptr;
        (void)ptx_dev_free(d_list);
        (void)ptx_dev_free(d_outw);
        d_list = nullptr;
        d_outw = nullptr;
        if (d_pack) { /* interior pointers: nothing of their own to free */
            (void)ptx_dev_free(d_pack);
            d_pack = nullptr;
            d_in_chg = d_in_op = d_out_off = d_doff = d_dcoff = nullptr;
            d_in_action = d_in_mt = nullptr;
            d_in_index = d_in_count = d_in_payload = d_in_values = d_actor = nullptr;
            d_list_off = nullptr;
        }
        (void)ptx_dev_free(d_list_off);
        d_list_off = nullptr;
        d_status = d_rows = d_chgs = nullptr; /* (parts of d_outw) */
        for (void* p : {(void*)d_in_chg, (void*)d_in_op, (void*)d_out_off, (void*)d_doff, (void*)d_dcoff, (void*)d_in_action, (void*)d_in_mt, (void*)d_in_index, (void*)d_in_count,
                        (void*)d_in_payload, (void*)d_in_values, (void*)d_actor, (void*)d_status, (void*)d_rows, (void*)d_chgs})
            (void)ptx_dev_free(p);
        d_in_chg = d_in_op = d_out_off = d_doff = d_dcoff = nullptr;
        d_in_action = d_in_mt = nullptr;
        d_in_index = d_in_count = d_in_payload = d_in_values = d_actor = d_status = d_rows = d_chgs = nullptr;
    };
#define PTX_TRYC(call)                                  \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string msg = std::string(#call) + ": " + hipGetErrorString(_e); \
            drop();                                     \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, msg); \
        }                                               \
    } while (0)
    auto up = [&](auto** dst, const auto* src, uint64_t count) -> hipError_t {
        hipError_t e = dalloc(dst, count);
        if (e == hipSuccess && count) e = hipMemcpyAsync(*dst, src, count * sizeof(**dst), hipMemcpyHostToDevice, ctx->stream);
        return e;
    };
    {
        /* the inputs of the call — an editor's edit is a few dozen bytes in eleven arrays — go up as ONE copy out of pinned memory where they are small (each
         * hipMemcpyAsync out of pageable memory was a staged, blocking copy of its own: ~0.1 ms of the 0.27 ms ptx_change took of a resident edit) */
        struct Piece {
            void** dst;
            const void* src;
            size_t bytes;
        };
        const Piece pieces[] = {{(void**)&d_in_chg, in->chg_off, ((size_t)L + 1) * 8}, {(void**)&d_in_op, in->op_off, ((size_t)NC + 1) * 8}, {(void**)&d_out_off, out_off.data(), ((size_t)L + 1) * 8},
                                {(void**)&d_list_off, list_off.data(), list_off[L] ? ((size_t)L + 1) * 8 : 0}, {(void**)&d_in_index, in->index, (size_t)NI * 4}, {(void**)&d_in_count, in->count, (size_t)NI * 4},
                                {(void**)&d_in_payload, in->payload, (size_t)NI * 4}, {(void**)&d_in_values, in->values, (size_t)in->n_values * 4}, {(void**)&d_actor, in->actor, (size_t)L * 4},
                                {(void**)&d_in_action, in->action, (size_t)NI}, {(void**)&d_in_mt, in->mark_type, (size_t)NI}};
        size_t total = 0;
        for (const Piece& q : pieces) total += (std::max<size_t>(q.bytes, 1) + 15) & ~(size_t)15;
        if (total <= (1u << 20)) {
            if (ctx->up_h_cap < total) {
                if (ctx->up_h) (void)hipHostFree(ctx->up_h);
                ctx->up_h = nullptr;
                ctx->up_h_cap = 0;
                PTX_TRYC(hipHostMalloc((void**)&ctx->up_h, 2 * total, hipHostMallocDefault));
                ctx->up_h_cap = 2 * total;
            }
            PTX_TRYC(ptx_dev_malloc((void**)&d_pack, total));
            size_t at = 0;
            for (const Piece& q : pieces) {
                if (q.bytes) memcpy(ctx->up_h + at, q.src, q.bytes);
                *q.dst = q.bytes || q.dst != (void**)&d_list_off ? (void*)(d_pack + at) : nullptr;
                at += (std::max<size_t>(q.bytes, 1) + 15) & ~(size_t)15;
            }
            PTX_TRYC(hipMemcpyAsync(d_pack, ctx->up_h, total, hipMemcpyHostToDevice, ctx->stream));
        } else {
            PTX_TRYC(up(&d_in_chg, in->chg_off, (uint64_t)L + 1));
            PTX_TRYC(up(&d_in_op, in->op_off, NC + 1));
            PTX_TRYC(up(&d_out_off, out_off.data(), (uint64_t)L + 1));
            PTX_TRYC(up(&d_in_action, in->action, NI));
            PTX_TRYC(up(&d_in_mt, in->mark_type, NI));
            PTX_TRYC(up(&d_in_index, in->index, NI));
            PTX_TRYC(up(&d_in_count, in->count, NI));
            PTX_TRYC(up(&d_in_payload, in->payload, NI));
            PTX_TRYC(up(&d_in_values, in->values, in->n_values));
            PTX_TRYC(up(&d_actor, in->actor, L));
            if (list_off[L]) PTX_TRYC(up(&d_list_off, list_off.data(), (uint64_t)L + 1));
        }
    }
    if (list_off[L]) PTX_TRYC(dalloc(&d_list, list_off[L]));
    PTX_TRYC(dalloc(&d_outw, 3 * (uint64_t)L + 1));
    d_status = d_outw;
    d_rows = d_outw + L;
    d_chgs = d_outw + 2 * (uint64_t)L;
    PTX_TRYC(dalloc(&cap->op_id, T));
    PTX_TRYC(dalloc(&cap->ref_a, T));
    PTX_TRYC(dalloc(&cap->ref_b, T));
    PTX_TRYC(dalloc(&cap->payload, T));
    PTX_TRYC(dalloc(&cap->action, T));
    PTX_TRYC(dalloc(&cap->mark_type, T));
    PTX_TRYC(dalloc(&cap->side_a, T));
    PTX_TRYC(dalloc(&cap->side_b, T));
    PTX_TRYC(dalloc(&cap->chg_hdr, NC));
    PTX_TRYC(dalloc(&cap->chg_env, NC * PTX_ENV_STRIDE(na)));
    PTX_TRYC(dalloc(&cap->chg_env_hi, NC * PTX_ENV_STRIDE(na) + 2));
    uint32_t* d_wide = d_outw + 3 * (uint64_t)L; /* the "some high half is set" word */
    uint32_t any_wide = 0;
    PTX_TRYC(hipMemsetAsync(d_wide, 0, 4, ctx->stream));
    std::vector<uint32_t> rows_made(std::max<uint32_t>(L, 1)), chgs_made(std::max<uint32_t>(L, 1));
    if (L) {
        PtxChangeArgs A;
        memset(&A, 0, sizeof(A));
        A.log_off = base->log_off;
        A.op_id = base->op_id;
        A.ref_a = base->ref_a;
        A.ref_b = base->ref_b;
        A.action = base->action;
        A.mark_type = base->mark_type;
        A.side_a = base->side_a;
        A.side_b = base->side_b;
        A.log_hdr = base->log_hdr;
        A.res = merged->logs;
        A.elem_rank = merged->rank;
        A.refs = merged->refs;
        A.refs_hi = merged->refs_hi;
        A.list_scratch = d_list;
        A.list_off = d_list_off;
        A.chg_off = base->chg_off;
        A.chg_hdr = base->chg_hdr;
        A.max_actors = na;
        A.in_chg_off = d_in_chg;
        A.in_op_off = d_in_op;
        A.in_action = d_in_action;
        A.in_mark_type = d_in_mt;
        A.in_index = d_in_index;
        A.in_count = d_in_count;
        A.in_payload = d_in_payload;
        A.in_values = d_in_values;
        A.actor = d_actor;
        A.out_off = d_out_off;
        A.o_op_id = cap->op_id;
        A.o_ref_a = cap->ref_a;
        A.o_ref_b = cap->ref_b;
        A.o_payload = cap->payload;
        A.o_action = cap->action;
        A.o_mark_type = cap->mark_type;
        A.o_side_a = cap->side_a;
        A.o_side_b = cap->side_b;
        A.o_chg_hdr = cap->chg_hdr;
        A.o_chg_env = cap->chg_env;
        A.o_chg_env_hi = cap->chg_env_hi;
        A.any_wide = d_wide;
        A.status = d_status;
        A.rows_made = d_rows;
        A.chgs_made = d_chgs;
        A.n_logs = L;
        A.lds_bytes = lds_bytes;
        hipLaunchKernelGGL(ptx_change_kernel, dim3(L), dim3(64), lds_bytes, ctx->stream, A);
        PTX_TRYC(hipGetLastError());
        std::vector<uint32_t> outw(3 * (size_t)L + 1);
        PTX_TRYC(hipMemcpyAsync(outw.data(), d_outw, outw.size() * 4, hipMemcpyDeviceToHost, ctx->stream)); /* one copy back: status, rows, changes, the flag */
        PTX_TRYC(hipStreamSynchronize(ctx->stream));
        memcpy(status_out, outw.data(), (size_t)L * 4);
        memcpy(rows_made.data(), outw.data() + L, (size_t)L * 4);
        memcpy(chgs_made.data(), outw.data() + 2 * (size_t)L, (size_t)L * 4);
        any_wide = outw[3 * (size_t)L];
    }
    /* the batch of what was made: failed logs contribute nothing */
    std::vector<uint64_t> doff((size_t)L + 1, 0), dcoff((size_t)L + 1, 0);
    for (uint32_t l = 0; l < L; ++l) {
        doff[l + 1] = doff[l] + rows_made[l];
        dcoff[l + 1] = dcoff[l] + chgs_made[l];
    }
    b = new ptx_dbatch();
    b->n_logs = L;
    b->n_ops = doff[L];
    b->max_actors = na;
    b->n_changes = dcoff[L];
    PTX_TRYC(up(&b->log_off, doff.data(), (uint64_t)L + 1));
    PTX_TRYC(up(&b->chg_off, dcoff.data(), (uint64_t)L + 1));
    PTX_TRYC(dalloc(&b->op_id, b->n_ops));
    PTX_TRYC(dalloc(&b->ref_a, b->n_ops));
    PTX_TRYC(dalloc(&b->ref_b, b->n_ops));
    PTX_TRYC(dalloc(&b->payload, b->n_ops));
    PTX_TRYC(dalloc(&b->action, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYC(dalloc(&b->mark_type, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYC(dalloc(&b->side_a, b->n_ops));
    PTX_TRYC(dalloc(&b->side_b, b->n_ops));
    PTX_TRYC(dalloc(&b->log_hdr, (uint64_t)L));
    PTX_TRYC(dalloc(&b->chg_hdr, b->n_changes + PTX_ENV_PAD));
    PTX_TRYC(dalloc(&b->chg_env, (b->n_changes + PTX_ENV_PAD) * PTX_ENV_STRIDE(na)));
    if (any_wide) PTX_TRYC(dalloc(&b->chg_env_hi, (b->n_changes + PTX_ENV_PAD) * PTX_ENV_STRIDE(na))); /* some new seq / dep is beyond 16 bits */
    if (L) {
        PtxAppendCols S = {cap->op_id, cap->ref_a, cap->ref_b, cap->payload, cap->action, cap->mark_type, cap->side_a, cap->side_b,
                           cap->chg_hdr, cap->chg_env, cap->chg_env_hi};
        PtxAppendDst D = {b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b, b->chg_hdr, b->chg_env, b->chg_env_hi};
        hipLaunchKernelGGL(ptx_take_rows_kernel, dim3(L), dim3(64), 0, ctx->stream, S, d_out_off, d_in_chg, d_rows, d_chgs, D, b->log_off, b->chg_off, na);
        PTX_TRYC(hipGetLastError());
        PTX_TRYC(hipStreamSynchronize(ctx->stream));
    }
#undef PTX_TRYC
    drop();
    const ptx_status st = census_and_shape(ctx, b, false);
    if (st != PTX_OK) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *made = b;
    return PTX_OK;
}

/* ---- InputOperations as a resident object, and change() from them (change_prep_core.h) ---- */
void ptx_input_ops_free(ptx_ctx* ctx, ptx_dinput_ops* d) {
    if (!d) return;
    if (ctx) (void)ptx_enter(ctx);
    if (d->owns)
        for (void* p : d->blocks) (void)ptx_dev_free(p);
    delete d;
}

ptx_status ptx_input_ops_upload(ptx_ctx* ctx, const ptx_input_ops* in, ptx_dinput_ops** out) {
    if (!ctx || !in || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    const uint32_t L = in->n_logs;
    if (L && (!in->chg_off || !in->op_off || !in->actor)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_input_ops_upload: chg_off / op_off / actor is NULL");
    /* the sizes, read where ptx_change reads them; nothing else is looked at (ptx_change_device checks on the device what ptx_change checks on the host) */
    const uint64_t NC = L ? in->chg_off[L] : 0;
    const uint64_t NI = NC ? in->op_off[NC] : 0;
    if (NI && (!in->action || !in->mark_type || !in->index || !in->count || !in->payload)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_input_ops_upload: an InputOperation column is NULL");
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_dinput_ops* d = new ptx_dinput_ops();
    d->n_logs = L;
    d->max_actors = in->max_actors;
    d->n_changes = NC;
    d->n_input_ops = NI;
    d->n_values = in->n_values;
    struct Piece {
        void** dst;
        const void* src;
        size_t bytes;
    };
    const Piece pieces[] = {{(void**)&d->chg_off, in->chg_off, in->chg_off ? ((size_t)L + 1) * 8 : 0}, {(void**)&d->op_off, in->op_off, in->op_off ? ((size_t)NC + 1) * 8 : 0}, {(void**)&d->index, in->index, (size_t)NI * 4},
                            {(void**)&d->count, in->count, (size_t)NI * 4}, {(void**)&d->payload, in->payload, (size_t)NI * 4},
                            {(void**)&d->values, in->values, in->values ? (size_t)in->n_values * 4 : 0}, {(void**)&d->actor, in->actor, (size_t)L * 4},
                            {(void**)&d->action, in->action, (size_t)NI}, {(void**)&d->mark_type, in->mark_type, (size_t)NI}};
    size_t total = 0;
    for (const Piece& q : pieces) total += (std::max<size_t>(q.bytes, 1) + 15) & ~(size_t)15;
    uint8_t* blk = nullptr;
    hipError_t e = ptx_dev_malloc((void**)&blk, total);
    d->blocks[0] = blk;
    const bool small = total <= (1u << 20); /* the eleven arrays of an edit go up as ONE copy out of pinned memory, as ptx_change sends them */
    if (e == hipSuccess && small && ctx->up_h_cap < total) {
        if (ctx->up_h) (void)hipHostFree(ctx->up_h);
        ctx->up_h = nullptr;
        ctx->up_h_cap = 0;
        e = hipHostMalloc((void**)&ctx->up_h, 2 * total, hipHostMallocDefault);
        if (e == hipSuccess) ctx->up_h_cap = 2 * total;
    }
    size_t at = 0;
    for (const Piece& q : pieces) {
        if (e != hipSuccess) break;
        /* a column the caller left NULL stays NULL (values: "an insert points outside `values`" is the device's to find), an empty one points at its own 16 bytes */
        *q.dst = q.src ? (void*)(blk + at) : nullptr;
        if (q.bytes && small) memcpy(ctx->up_h + at, q.src, q.bytes);
        else if (q.bytes) e = hipMemcpyAsync(blk + at, q.src, q.bytes, hipMemcpyHostToDevice, ctx->stream);
        at += (std::max<size_t>(q.bytes, 1) + 15) & ~(size_t)15;
    }
    if (e == hipSuccess && small) e = hipMemcpyAsync(blk, ctx->up_h, total, hipMemcpyHostToDevice, ctx->stream);
    { /* the caller's arrays and the staging block are free to go when the call returns */
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = e2;
    }
    if (e != hipSuccess) {
        ptx_input_ops_free(ctx, d);
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_input_ops_upload: ") + hipGetErrorString(e));
    }
    *out = d;
    return PTX_OK;
}

ptx_status ptx_input_ops_wrap_device(ptx_ctx* ctx, const ptx_input_ops* dev, uint64_t n_changes, uint64_t n_input_ops, ptx_dinput_ops** out) {
    if (!ctx || !dev || !out) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    ptx_dinput_ops* d = new ptx_dinput_ops();
    d->owns = false;
    d->n_logs = dev->n_logs;
    d->max_actors = dev->max_actors;
    d->n_changes = n_changes;
    d->n_input_ops = n_input_ops;
    d->n_values = dev->n_values;
    d->chg_off = (uint64_t*)dev->chg_off;
    d->op_off = (uint64_t*)dev->op_off;
    d->action = (uint8_t*)dev->action;
    d->mark_type = (uint8_t*)dev->mark_type;
    d->index = (uint32_t*)dev->index;
    d->count = (uint32_t*)dev->count;
    d->payload = (uint32_t*)dev->payload;
    d->values = (uint32_t*)dev->values;
    d->actor = (uint32_t*)dev->actor;
    *out = d;
    return PTX_OK;
}

struct PtxHostInputOpsOwner {
    uint8_t* block = nullptr;
    ~PtxHostInputOpsOwner() { free(block); }
};
void ptx_host_input_ops_free(ptx_host_input_ops* h) {
    if (!h) return;
    delete (PtxHostInputOpsOwner*)h->owner;
    memset(h, 0, sizeof(*h));
}
ptx_status ptx_input_ops_download(ptx_ctx* ctx, const ptx_dinput_ops* d, ptx_host_input_ops* out) {
    if (!ctx || !d || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    const uint32_t L = d->n_logs;
    const uint64_t NC = d->n_changes, NI = d->n_input_ops;
    if (L && (!d->chg_off || !d->op_off || !d->actor)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_input_ops_download: chg_off / op_off / actor is NULL");
    if (NI && (!d->action || !d->mark_type || !d->index || !d->count || !d->payload)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_input_ops_download: an InputOperation column is NULL");
    PTX_HIP(ctx, ptx_enter(ctx));
    struct Piece {
        const void** dst;
        const void* src;
        size_t bytes;
    };
    ptx_input_ops& o = out->ops;
    const Piece pieces[] = {{(const void**)&o.chg_off, d->chg_off, d->chg_off ? ((size_t)L + 1) * 8 : 0}, {(const void**)&o.op_off, d->op_off, d->op_off ? ((size_t)NC + 1) * 8 : 0}, {(const void**)&o.index, d->index, (size_t)NI * 4},
                            {(const void**)&o.count, d->count, (size_t)NI * 4}, {(const void**)&o.payload, d->payload, (size_t)NI * 4},
                            {(const void**)&o.values, d->values, d->values ? (size_t)d->n_values * 4 : 0}, {(const void**)&o.actor, d->actor, (size_t)L * 4},
                            {(const void**)&o.action, d->action, (size_t)NI}, {(const void**)&o.mark_type, d->mark_type, (size_t)NI}};
    size_t total = 0;
    for (const Piece& q : pieces) total += (std::max<size_t>(q.bytes, 1) + 15) & ~(size_t)15;
    PtxHostInputOpsOwner* own = new PtxHostInputOpsOwner();
    own->block = (uint8_t*)calloc(total, 1);
    hipError_t e = own->block ? hipSuccess : hipErrorOutOfMemory;
    size_t at = 0;
    for (const Piece& q : pieces) {
        if (e != hipSuccess) break;
        *q.dst = q.src ? (const void*)(own->block + at) : nullptr;
        if (q.bytes) e = hipMemcpyAsync(own->block + at, q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream);
        at += (std::max<size_t>(q.bytes, 1) + 15) & ~(size_t)15;
    }
    {
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = e2;
    }
    if (e != hipSuccess) {
        delete own;
        memset(out, 0, sizeof(*out));
        return fail(ctx, e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, std::string("ptx_input_ops_download: ") + hipGetErrorString(e));
    }
    o.n_logs = L;
    o.max_actors = d->max_actors;
    o.n_values = d->n_values;
    out->n_changes = NC;
    out->n_input_ops = NI;
    out->owner = own;
    return PTX_OK;
}

/* ptx_change for resident InputOperations.  Three waits: the verdict of the prepare passes with the totals and the LDS need; the per-log status with the sizes
 * of the made batch; the made batch.  Between them nothing proportional to the ops or to the base batch's logs crosses PCIe except status_out */
ptx_status ptx_change_device(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_dresult* merged, const ptx_dinput_ops* in, ptx_dbatch** made, uint32_t* status_out) {
    if (!ctx || !base || !merged || !in || !made || !status_out) return PTX_ERR_INVALID_ARG;
    *made = nullptr;
    const uint32_t L = base->n_logs;
    if (in->n_logs != L) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: the InputOperations must name every log of the base batch (a log may make no change)");
    if (merged->n_logs != L || merged->n_rows != base->n_ops) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: `merged` is not the result of this batch");
    if (!merged->rank) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change needs the elem_rank column (context created with PTX_FLAG_NO_ELEM_RANK)");
    if (L && (!in->chg_off || !in->op_off || !in->actor)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: chg_off / op_off / actor is NULL");
    if (base->n_ops && !base->chg_off) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change needs the Change envelope of the base batch (the replicas' clocks)");
    const uint32_t na = base->chg_off && base->n_changes ? base->max_actors : in->max_actors;
    if (na == 0 || na > 4096u || (base->chg_off && base->n_changes && in->max_actors && in->max_actors != base->max_actors))
        return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: max_actors must be 1..4096 and equal to the base batch's");
    const uint64_t NC = L ? in->n_changes : 0;
    const uint64_t NI = NC ? in->n_input_ops : 0;
    if (NI && (!in->action || !in->mark_type || !in->index || !in->count || !in->payload)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_change: an InputOperation column is NULL");
    PTX_HIP(ctx, ptx_enter(ctx));

    /* work block: err | lds_need | rows [L] | list_words [L] | out_off [L + 1] | list_off [L + 1] */
    auto a16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t rows_at = 16, lw_at = rows_at + a16((uint64_t)L * 4), oo_at = lw_at + a16((uint64_t)L * 4), lo_at = oo_at + a16(((uint64_t)L + 1) * 8), wbytes = lo_at + a16(((uint64_t)L + 1) * 8);
    uint8_t* d_work = nullptr;
    ptx_dbatch* cap = new ptx_dbatch(); /* the kernel's capacity-layout output, owned here */
    ptx_dbatch* b = nullptr;
    uint32_t *d_list = nullptr, *d_outw = nullptr;
    auto drop = [&]() {
        ptx_batch_free(ctx, cap);
        cap = nullptr;
        (void)ptx_dev_free(d_work);
        (void)ptx_dev_free(d_list);
        (void)ptx_dev_free(d_outw);
        d_work = nullptr;
        d_list = d_outw = nullptr;
    };
#define PTX_TRYD(call)                                  \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string msg = std::string(#call) + ": " + hipGetErrorString(_e); \
            drop();                                     \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, msg); \
        }                                               \
    } while (0)
    if (ctx->up_h_cap < 64) { /* the small blocks that come down land in the context's pinned staging */
        if (ctx->up_h) (void)hipHostFree(ctx->up_h);
        ctx->up_h = nullptr;
        ctx->up_h_cap = 0;
        PTX_TRYD(hipHostMalloc((void**)&ctx->up_h, 4096, hipHostMallocDefault));
        ctx->up_h_cap = 4096;
    }
    uint64_t* down = (uint64_t*)ctx->up_h; /* [0] err, [1] lds_need, [2] total rows, [3] total list words; later [0] rows made, [1] changes made, [2] the wide flag */
    PTX_TRYD(ptx_dev_malloc((void**)&d_work, wbytes));
    uint32_t* d_rows_need = (uint32_t*)(d_work + rows_at);
    uint32_t* d_list_words = (uint32_t*)(d_work + lw_at);
    uint64_t* d_out_off = (uint64_t*)(d_work + oo_at);
    uint64_t* d_list_off = (uint64_t*)(d_work + lo_at);
    uint64_t T = 0, list_total = 0, need = 4096;
    if (L) {
        PTX_TRYD(hipMemsetAsync(d_work, 0xFF, 8, ctx->stream));
        PTX_TRYD(hipMemsetAsync(d_work + 8, 0, 8, ctx->stream));
        PtxChangePrepArgs P;
        memset(&P, 0, sizeof(P));
        P.chg_off = in->chg_off;
        P.op_off = in->op_off;
        P.action = in->action;
        P.count = in->count;
        P.payload = in->payload;
        P.n_changes = in->n_changes;
        P.n_input_ops = in->n_input_ops;
        P.n_values = in->n_values;
        P.has_values = in->values ? 1u : 0u;
        P.n_logs = L;
        P.log_off = base->log_off;
        P.log_hdr = base->log_hdr;
        P.max_actors = na;
        P.all_in_hbm = getenv("PTX_CHANGE_LIST_IN_HBM") != nullptr ? 1u : 0u; /* (tests: the list of EVERY log in global scratch) */
        P.max_lds = ctx->max_lds;
        P.rows = d_rows_need;
        P.list_words = d_list_words;
        P.err = (unsigned long long*)d_work;
        P.lds_need = (unsigned long long*)(d_work + 8);
        const uint64_t entries = ptx_change_offsets_entries(P);
        hipLaunchKernelGGL(ptx_change_offsets_check_kernel, dim3((uint32_t)((entries + 255) / 256)), dim3(256), 0, ctx->stream, P);
        hipLaunchKernelGGL(ptx_change_prep_kernel, dim3(L), dim3(64), 0, ctx->stream, P);
        hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)d_rows_need, 0xFFFFFFFFu, d_out_off, L);
        hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)d_list_words, 0xFFFFFFFFu, d_list_off, L);
        PTX_TRYD(hipGetLastError());
        PTX_TRYD(hipMemcpyAsync(down, d_work, 16, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipMemcpyAsync(down + 2, d_out_off + L, 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipMemcpyAsync(down + 3, d_list_off + L, 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipStreamSynchronize(ctx->stream)); /* the verdict: before any output is allocated */
        const uint64_t err = down[0];
        if (err != PTX_CP_NO_ERROR) {
            const uint32_t code = (uint32_t)(err >> 56);
            const unsigned long long at = err & PTX_CP_AT_MASK;
            drop();
            std::string msg;
            if (code == PTX_CP_CHG_START) msg = "ptx_change: chg_off must start at 0";
            else if (code == PTX_CP_CHG_ORDER) msg = "ptx_change: chg_off decreases at entry " + std::to_string(at);
            else if (code == PTX_CP_OP_START) msg = "ptx_change: op_off must start at 0";
            else if (code == PTX_CP_OP_ORDER) msg = "ptx_change: op_off decreases at entry " + std::to_string(at);
            else if (code == PTX_CP_SIZES) msg = std::string("ptx_change: ") + (at ? "op_off" : "chg_off") + " does not end at the size the InputOperations were wrapped with";
            else if (code == PTX_CP_VALUES) msg = "ptx_change: an insert points outside `values` (log " + std::to_string(at) + ")";
            else msg = "ptx_change: more than 65534 ops for one log (log " + std::to_string(at) + ")";
            return fail(ctx, PTX_ERR_INVALID_ARG, msg);
        }
        need = std::max<uint64_t>(need, down[1]);
        T = down[2];
        list_total = down[3];
    }
    const uint32_t lds_bytes = (uint32_t)std::min<uint64_t>((need + 255) & ~255ull, ctx->max_lds); /* larger logs report PTX_ERR_CAPACITY */

    if (list_total) PTX_TRYD(dalloc(&d_list, list_total));
    PTX_TRYD(dalloc(&d_outw, 3 * (uint64_t)L + 1));
    uint32_t *d_status = d_outw, *d_rows = d_outw + L, *d_chgs = d_outw + 2 * (uint64_t)L, *d_wide = d_outw + 3 * (uint64_t)L;
    PTX_TRYD(dalloc(&cap->op_id, T));
    PTX_TRYD(dalloc(&cap->ref_a, T));
    PTX_TRYD(dalloc(&cap->ref_b, T));
    PTX_TRYD(dalloc(&cap->payload, T));
    PTX_TRYD(dalloc(&cap->action, T));
    PTX_TRYD(dalloc(&cap->mark_type, T));
    PTX_TRYD(dalloc(&cap->side_a, T));
    PTX_TRYD(dalloc(&cap->side_b, T));
    PTX_TRYD(dalloc(&cap->chg_hdr, NC));
    PTX_TRYD(dalloc(&cap->chg_env, NC * PTX_ENV_STRIDE(na)));
    PTX_TRYD(dalloc(&cap->chg_env_hi, NC * PTX_ENV_STRIDE(na) + 2));
    PTX_TRYD(hipMemsetAsync(d_wide, 0, 4, ctx->stream));
    b = new ptx_dbatch();
    b->n_logs = L;
    b->max_actors = na;
    PTX_TRYD(dalloc(&b->log_off, (uint64_t)L + 1));
    PTX_TRYD(dalloc(&b->chg_off, (uint64_t)L + 1));
    uint32_t any_wide = 0;
    if (L) {
        PtxChangeArgs A;
        memset(&A, 0, sizeof(A));
        A.log_off = base->log_off;
        A.op_id = base->op_id;
        A.ref_a = base->ref_a;
        A.ref_b = base->ref_b;
        A.action = base->action;
        A.mark_type = base->mark_type;
        A.side_a = base->side_a;
        A.side_b = base->side_b;
        A.log_hdr = base->log_hdr;
        A.res = merged->logs;
        A.elem_rank = merged->rank;
        A.refs = merged->refs;
        A.refs_hi = merged->refs_hi;
        A.list_scratch = d_list;
        A.list_off = d_list ? d_list_off : nullptr;
        A.chg_off = base->chg_off;
        A.chg_hdr = base->chg_hdr;
        A.max_actors = na;
        A.in_chg_off = in->chg_off;
        A.in_op_off = in->op_off;
        A.in_action = in->action;
        A.in_mark_type = in->mark_type;
        A.in_index = in->index;
        A.in_count = in->count;
        A.in_payload = in->payload;
        A.in_values = in->values;
        A.actor = in->actor;
        A.out_off = d_out_off;
        A.o_op_id = cap->op_id;
        A.o_ref_a = cap->ref_a;
        A.o_ref_b = cap->ref_b;
        A.o_payload = cap->payload;
        A.o_action = cap->action;
        A.o_mark_type = cap->mark_type;
        A.o_side_a = cap->side_a;
        A.o_side_b = cap->side_b;
        A.o_chg_hdr = cap->chg_hdr;
        A.o_chg_env = cap->chg_env;
        A.o_chg_env_hi = cap->chg_env_hi;
        A.any_wide = d_wide;
        A.status = d_status;
        A.rows_made = d_rows;
        A.chgs_made = d_chgs;
        A.n_logs = L;
        A.lds_bytes = lds_bytes;
        hipLaunchKernelGGL(ptx_change_kernel, dim3(L), dim3(64), lds_bytes, ctx->stream, A);
        /* the offsets of the made batch: failed logs contribute nothing */
        hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)d_rows, 0xFFFFFFFFu, b->log_off, L);
        hipLaunchKernelGGL(ptx_find_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)d_chgs, 0xFFFFFFFFu, b->chg_off, L);
        PTX_TRYD(hipGetLastError());
        PTX_TRYD(hipMemcpyAsync(status_out, d_status, (size_t)L * 4, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipMemcpyAsync(down, b->log_off + L, 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipMemcpyAsync(down + 1, b->chg_off + L, 8, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipMemcpyAsync(down + 2, d_wide, 4, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYD(hipStreamSynchronize(ctx->stream));
        b->n_ops = down[0];
        b->n_changes = down[1];
        any_wide = (uint32_t)down[2];
    } else {
        PTX_TRYD(hipMemsetAsync(b->log_off, 0, 8, ctx->stream));
        PTX_TRYD(hipMemsetAsync(b->chg_off, 0, 8, ctx->stream));
    }
    PTX_TRYD(dalloc(&b->op_id, b->n_ops));
    PTX_TRYD(dalloc(&b->ref_a, b->n_ops));
    PTX_TRYD(dalloc(&b->ref_b, b->n_ops));
    PTX_TRYD(dalloc(&b->payload, b->n_ops));
    PTX_TRYD(dalloc(&b->action, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYD(dalloc(&b->mark_type, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYD(dalloc(&b->side_a, b->n_ops));
    PTX_TRYD(dalloc(&b->side_b, b->n_ops));
    PTX_TRYD(dalloc(&b->log_hdr, (uint64_t)L));
    PTX_TRYD(dalloc(&b->chg_hdr, b->n_changes + PTX_ENV_PAD));
    PTX_TRYD(dalloc(&b->chg_env, (b->n_changes + PTX_ENV_PAD) * PTX_ENV_STRIDE(na)));
    if (any_wide) PTX_TRYD(dalloc(&b->chg_env_hi, (b->n_changes + PTX_ENV_PAD) * PTX_ENV_STRIDE(na))); /* some new seq / dep is beyond 16 bits */
    if (L) {
        PtxAppendCols S = {cap->op_id, cap->ref_a, cap->ref_b, cap->payload, cap->action, cap->mark_type, cap->side_a, cap->side_b,
                           cap->chg_hdr, cap->chg_env, cap->chg_env_hi};
        PtxAppendDst D = {b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b, b->chg_hdr, b->chg_env, b->chg_env_hi};
        hipLaunchKernelGGL(ptx_take_rows_kernel, dim3(L), dim3(64), 0, ctx->stream, S, d_out_off, in->chg_off, d_rows, d_chgs, D, b->log_off, b->chg_off, na);
        PTX_TRYD(hipGetLastError());
        PTX_TRYD(hipStreamSynchronize(ctx->stream));
    }
#undef PTX_TRYD
    drop();
    const ptx_status st = census_and_shape(ctx, b, false);
    if (st != PTX_OK) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *made = b;
    return PTX_OK;
}

/* ---- sync of replica logs: the missing changes of every (source, target) pair in retry order (sync_core.h) ---- */
ptx_status ptx_sync_replicas(ptx_ctx* ctx, const ptx_dbatch* base, uint32_t n_pairs, const uint32_t* src_log, const uint32_t* dst_log, uint32_t max_attempts, ptx_dbatch** more,
                             uint32_t* status_out) {
    if (!ctx || !base || !more || (n_pairs && (!src_log || !dst_log || !status_out))) return PTX_ERR_INVALID_ARG;
    *more = nullptr;
    const uint32_t L = base->n_logs, P = n_pairs, na = base->max_actors;
    if (!base->chg_off || !base->chg_hdr || !base->chg_env || na == 0) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_sync_replicas needs the Change envelope of the batch (the replicas' clocks)");
    {
        std::vector<uint8_t> is_target(std::max<uint32_t>(L, 1), 0);
        const int bad = ptx_sync_check_pairs(L, P, src_log, dst_log, is_target.data());
        if (bad == 1) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_sync_replicas: a pair names a log the batch does not have");
        if (bad == 2) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_sync_replicas: a log is the target of two pairs (a target log takes one source per call)");
    }
    const uint64_t lds_need = (ptx_sync_lds_need(na) + 255) & ~255ull;
    if (lds_need > ctx->max_lds) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_sync_replicas: the per-actor tables of max_actors do not fit one CU's LDS");
    PTX_HIP(ctx, ptx_enter(ctx));
    /* the pinned staging block of the context's small uploads, grown on demand */
    auto staging = [&](size_t bytes) -> hipError_t {
        if (ctx->up_h_cap >= bytes) return hipSuccess;
        if (ctx->up_h) (void)hipHostFree(ctx->up_h);
        ctx->up_h = nullptr;
        ctx->up_h_cap = 0;
        hipError_t e = hipHostMalloc((void**)&ctx->up_h, 2 * bytes, hipHostMallocDefault);
        if (e == hipSuccess) ctx->up_h_cap = 2 * bytes;
        return e;
    };
    uint8_t *d_in = nullptr, *d_off = nullptr;
    uint32_t *d_scratch = nullptr, *d_out = nullptr;
    ptx_dbatch* b = nullptr;
    auto drop = [&]() {
        (void)ptx_dev_free(d_in);
        (void)ptx_dev_free(d_off);
        (void)ptx_dev_free(d_scratch);
        (void)ptx_dev_free(d_out);
        d_in = d_off = nullptr;
        d_scratch = d_out = nullptr;
    };
#define PTX_TRYS(call)                                  \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string msg = std::string(#call) + ": " + hipGetErrorString(_e); \
            drop();                                     \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, msg); \
        }                                               \
    } while (0)
    /* the envelope offsets of the base size the scratch slices: one small copy through the pinned block */
    const size_t off_bytes = ((size_t)L + 1) * 8, pair_bytes = ((size_t)P * 4 + 15) & ~(size_t)15, scr_bytes = ((size_t)P + 1) * 8;
    const size_t in_bytes = 2 * pair_bytes + scr_bytes;
    PTX_TRYS(staging(std::max(std::max(off_bytes, in_bytes), 2 * off_bytes)));
    PTX_TRYS(hipMemcpyAsync(ctx->up_h, base->chg_off, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PTX_TRYS(hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> coff((size_t)L + 1), scr((size_t)P + 1, 0);
    memcpy(coff.data(), ctx->up_h, off_bytes);
    for (uint32_t p = 0; p < P; ++p) scr[p + 1] = scr[p] + ptx_sync_scratch_words(coff[src_log[p] + 1] - coff[src_log[p]]);
    std::vector<uint32_t> outw(3 * (size_t)P + 1, 0);
    if (P) {
        PTX_TRYS(ptx_dev_malloc((void**)&d_in, in_bytes));
        PTX_TRYS(dalloc(&d_scratch, scr[P]));
        PTX_TRYS(dalloc(&d_out, 3 * (uint64_t)P));
        memcpy(ctx->up_h, src_log, (size_t)P * 4);
        memcpy(ctx->up_h + pair_bytes, dst_log, (size_t)P * 4);
        memcpy(ctx->up_h + 2 * pair_bytes, scr.data(), scr_bytes);
        PTX_TRYS(hipMemcpyAsync(d_in, ctx->up_h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    PtxSyncArgs A;
    memset(&A, 0, sizeof(A));
    A.log_off = base->log_off;
    A.chg_off = base->chg_off;
    A.chg_hdr = base->chg_hdr;
    A.chg_env = base->chg_env;
    A.chg_env_hi = base->chg_env_hi;
    A.max_actors = na;
    A.n_pairs = P;
    A.max_attempts = max_attempts;
    A.src_log = (const uint32_t*)d_in;
    A.dst_log = (const uint32_t*)(d_in + pair_bytes);
    A.scr_off = (const uint64_t*)(d_in + 2 * pair_bytes);
    A.scratch = d_scratch;
    A.status = d_out;
    A.n_admitted = d_out + P;
    A.n_rows = d_out + 2 * (size_t)P;
    A.lds_bytes = (uint32_t)lds_need;
    if (P) {
        hipLaunchKernelGGL(ptx_sync_plan_kernel, dim3(P), dim3(64), (uint32_t)lds_need, ctx->stream, A);
        PTX_TRYS(hipGetLastError());
        /* one copy back: status, admitted changes and rows of every pair */
        PTX_TRYS(staging(3 * (size_t)P * 4));
        PTX_TRYS(hipMemcpyAsync(ctx->up_h, d_out, 3 * (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYS(hipStreamSynchronize(ctx->stream));
        memcpy(outw.data(), ctx->up_h, 3 * (size_t)P * 4);
        memcpy(status_out, outw.data(), (size_t)P * 4);
    }
    /* `more`: log dst_log[p] = the admitted changes of pair p, every other log empty */
    std::vector<uint64_t> doff((size_t)L + 1, 0), dcoff((size_t)L + 1, 0);
    for (uint32_t p = 0; p < P; ++p) {
        dcoff[(size_t)dst_log[p] + 1] = outw[(size_t)P + p];
        doff[(size_t)dst_log[p] + 1] = outw[2 * (size_t)P + p];
    }
    for (uint32_t l = 0; l < L; ++l) {
        doff[l + 1] += doff[l];
        dcoff[l + 1] += dcoff[l];
    }
    b = new ptx_dbatch();
    b->n_logs = L;
    b->n_ops = doff[L];
    b->max_actors = na;
    b->n_changes = dcoff[L];
    const uint64_t ES = PTX_ENV_STRIDE(na);
    PTX_TRYS(dalloc(&b->log_off, (uint64_t)L + 1));
    PTX_TRYS(dalloc(&b->chg_off, (uint64_t)L + 1));
    PTX_TRYS(staging(2 * off_bytes));
    memcpy(ctx->up_h, doff.data(), off_bytes);
    memcpy(ctx->up_h + off_bytes, dcoff.data(), off_bytes);
    PTX_TRYS(hipMemcpyAsync(b->log_off, ctx->up_h, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    PTX_TRYS(hipMemcpyAsync(b->chg_off, ctx->up_h + off_bytes, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    PTX_TRYS(dalloc(&b->op_id, b->n_ops));
    PTX_TRYS(dalloc(&b->ref_a, b->n_ops));
    PTX_TRYS(dalloc(&b->ref_b, b->n_ops));
    PTX_TRYS(dalloc(&b->payload, b->n_ops));
    PTX_TRYS(dalloc(&b->action, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYS(dalloc(&b->mark_type, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYS(dalloc(&b->side_a, b->n_ops));
    PTX_TRYS(dalloc(&b->side_b, b->n_ops));
    PTX_TRYS(dalloc(&b->log_hdr, (uint64_t)L));
    PTX_TRYS(dalloc(&b->chg_hdr, b->n_changes + PTX_ENV_PAD));
    PTX_TRYS(dalloc(&b->chg_env, (b->n_changes + PTX_ENV_PAD) * ES));
    if (base->chg_env_hi) PTX_TRYS(dalloc(&b->chg_env_hi, (b->n_changes + PTX_ENV_PAD) * ES));
    if (P && b->n_changes) {
        PtxSyncGatherArgs G = {base->op_id, base->ref_a, base->ref_b, base->payload, base->action, base->mark_type, base->side_a, base->side_b,
                               b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b,
                               b->chg_hdr, b->chg_env, b->chg_env_hi, b->log_off, b->chg_off};
        hipLaunchKernelGGL(ptx_sync_gather_kernel, dim3(P), dim3(PTX_SYNC_GATHER_THREADS), 0, ctx->stream, A, G);
        PTX_TRYS(hipGetLastError());
    }
    PTX_TRYS(hipStreamSynchronize(ctx->stream));
#undef PTX_TRYS
    drop();
    const ptx_status st = census_and_shape(ctx, b, false);
    if (st != PTX_OK) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *more = b;
    return PTX_OK;
}

/* ---- resident logs at a past version: the kept changes of every cut, optionally the rest behind them (version_core.h) ---- */
ptx_status ptx_batch_at_versions(ptx_ctx* ctx, const ptx_dbatch* base, uint32_t n_cuts, const uint32_t* src_log, const uint32_t* clocks, const uint32_t* prefix, uint32_t flags,
                                 ptx_dbatch** out, uint32_t* status_out, uint32_t* n_kept_out, uint32_t* first_row_out, uint32_t* clocks_out) {
    if (!ctx || !base || !out || (n_cuts && (!src_log || !status_out))) return PTX_ERR_INVALID_ARG;
    *out = nullptr;
    const uint32_t L = base->n_logs, P = n_cuts, na = base->max_actors;
    if (!base->chg_off || !base->chg_hdr || !base->chg_env || na == 0) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_at_versions needs the Change envelope of the batch (the changes' seqs and deps)");
    if (P && (clocks != nullptr) == (prefix != nullptr)) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_at_versions takes clock cuts or prefix cuts, one of the two");
    if (flags & ~PTX_VERSIONS_THEN_REST) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_at_versions: unknown flag");
    for (uint32_t c = 0; c < P; ++c)
        if (src_log[c] >= L) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_at_versions: a cut names a log the batch does not have");
    const uint64_t lds_need = (ptx_version_lds_need(na) + 255) & ~255ull;
    if (lds_need > ctx->max_lds) return fail(ctx, PTX_ERR_INVALID_ARG, "ptx_batch_at_versions: the per-actor clocks of max_actors do not fit one CU's LDS");
    PTX_HIP(ctx, ptx_enter(ctx));
    auto staging = [&](size_t bytes) -> hipError_t { /* the pinned staging block of the context's small uploads, grown on demand */
        if (ctx->up_h_cap >= bytes) return hipSuccess;
        if (ctx->up_h) (void)hipHostFree(ctx->up_h);
        ctx->up_h = nullptr;
        ctx->up_h_cap = 0;
        hipError_t e = hipHostMalloc((void**)&ctx->up_h, 2 * bytes, hipHostMallocDefault);
        if (e == hipSuccess) ctx->up_h_cap = 2 * bytes;
        return e;
    };
    uint8_t* d_in = nullptr;
    uint32_t *d_scratch = nullptr, *d_out = nullptr;
    ptx_dbatch* b = nullptr;
    auto drop = [&]() {
        (void)ptx_dev_free(d_in);
        (void)ptx_dev_free(d_scratch);
        (void)ptx_dev_free(d_out);
        d_in = nullptr;
        d_scratch = d_out = nullptr;
    };
#define PTX_TRYV(call)                                  \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) {                         \
            std::string msg = std::string(#call) + ": " + hipGetErrorString(_e); \
            drop();                                     \
            ptx_batch_free(ctx, b);                     \
            return fail(ctx, _e == hipErrorOutOfMemory ? PTX_ERR_OOM : PTX_ERR_HIP, msg); \
        }                                               \
    } while (0)
    /* the envelope offsets of the base size the scratch slices: one small copy through the pinned block */
    const size_t off_bytes = ((size_t)L + 1) * 8, cut_bytes = ((size_t)P * 4 + 15) & ~(size_t)15, scr_bytes = ((size_t)P + 1) * 8;
    const size_t want_bytes = clocks ? (size_t)P * na * 4 : (size_t)P * 4;
    const size_t in_bytes = 2 * cut_bytes + scr_bytes + want_bytes;  /* src_log | dst_log | scr_off | clocks or prefix */
    const size_t out_words = (5 + (size_t)na) * P;                   /* status | changes | rows | n_kept | first_row | clocks_out */
    PTX_TRYV(staging(std::max(off_bytes, std::max(in_bytes, out_words * 4))));
    PTX_TRYV(hipMemcpyAsync(ctx->up_h, base->chg_off, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PTX_TRYV(hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> scr((size_t)P + 1, 0);
    {
        const uint64_t* coff = (const uint64_t*)ctx->up_h;
        for (uint32_t c = 0; c < P; ++c) scr[c + 1] = scr[c] + ptx_sync_scratch_words(coff[src_log[c] + 1] - coff[src_log[c]]);
    }
    std::vector<uint32_t> outw(out_words + 1, 0);
    PtxVersionArgs V;
    memset(&V, 0, sizeof(V));
    PtxSyncArgs& A = V.S;
    if (P) {
        PTX_TRYV(ptx_dev_malloc((void**)&d_in, in_bytes));
        PTX_TRYV(dalloc(&d_scratch, scr[P]));
        PTX_TRYV(dalloc(&d_out, (uint64_t)out_words));
        memcpy(ctx->up_h, src_log, (size_t)P * 4);
        for (uint32_t c = 0; c < P; ++c) ((uint32_t*)(ctx->up_h + cut_bytes))[c] = c; /* log c of *out is cut c */
        memcpy(ctx->up_h + 2 * cut_bytes, scr.data(), scr_bytes);
        memcpy(ctx->up_h + 2 * cut_bytes + scr_bytes, clocks ? clocks : prefix, want_bytes);
        PTX_TRYV(hipMemcpyAsync(d_in, ctx->up_h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    A.log_off = base->log_off;
    A.chg_off = base->chg_off;
    A.chg_hdr = base->chg_hdr;
    A.chg_env = base->chg_env;
    A.chg_env_hi = base->chg_env_hi;
    A.max_actors = na;
    A.n_pairs = P;
    A.src_log = (const uint32_t*)d_in;
    A.dst_log = (const uint32_t*)(d_in + cut_bytes);
    A.scr_off = (const uint64_t*)(d_in + 2 * cut_bytes);
    A.scratch = d_scratch;
    A.status = d_out;
    A.n_admitted = d_out + P;
    A.n_rows = d_out + 2 * (size_t)P;
    A.lds_bytes = (uint32_t)lds_need;
    V.clocks = clocks ? (const uint32_t*)(d_in + 2 * cut_bytes + scr_bytes) : nullptr;
    V.prefix = clocks ? nullptr : (const uint32_t*)(d_in + 2 * cut_bytes + scr_bytes);
    V.flags = flags;
    V.n_kept = d_out + 3 * (size_t)P;
    V.first_row = d_out + 4 * (size_t)P;
    V.clocks_out = d_out + 5 * (size_t)P;
    if (P) {
        hipLaunchKernelGGL(ptx_version_plan_kernel, dim3(P), dim3(64), (uint32_t)lds_need, ctx->stream, V);
        PTX_TRYV(hipGetLastError());
        /* one copy back: the totals and the effective clock of every cut */
        PTX_TRYV(hipMemcpyAsync(ctx->up_h, d_out, out_words * 4, hipMemcpyDeviceToHost, ctx->stream));
        PTX_TRYV(hipStreamSynchronize(ctx->stream));
        memcpy(outw.data(), ctx->up_h, out_words * 4);
        memcpy(status_out, outw.data(), (size_t)P * 4);
        if (n_kept_out) memcpy(n_kept_out, outw.data() + 3 * (size_t)P, (size_t)P * 4);
        if (first_row_out) memcpy(first_row_out, outw.data() + 4 * (size_t)P, (size_t)P * 4);
        if (clocks_out) memcpy(clocks_out, outw.data() + 5 * (size_t)P, (size_t)P * na * 4);
    }
    /* *out: log c = cut c */
    std::vector<uint64_t> doff((size_t)P + 1, 0), dcoff((size_t)P + 1, 0);
    for (uint32_t c = 0; c < P; ++c) {
        dcoff[c + 1] = dcoff[c] + outw[(size_t)P + c];
        doff[c + 1] = doff[c] + outw[2 * (size_t)P + c];
    }
    b = new ptx_dbatch();
    b->n_logs = P;
    b->n_ops = doff[P];
    b->max_actors = na;
    b->n_changes = dcoff[P];
    const uint64_t ES = PTX_ENV_STRIDE(na);
    const size_t poff_bytes = ((size_t)P + 1) * 8;
    PTX_TRYV(dalloc(&b->log_off, (uint64_t)P + 1));
    PTX_TRYV(dalloc(&b->chg_off, (uint64_t)P + 1));
    PTX_TRYV(staging(2 * poff_bytes));
    memcpy(ctx->up_h, doff.data(), poff_bytes);
    memcpy(ctx->up_h + poff_bytes, dcoff.data(), poff_bytes);
    PTX_TRYV(hipMemcpyAsync(b->log_off, ctx->up_h, poff_bytes, hipMemcpyHostToDevice, ctx->stream));
    PTX_TRYV(hipMemcpyAsync(b->chg_off, ctx->up_h + poff_bytes, poff_bytes, hipMemcpyHostToDevice, ctx->stream));
    PTX_TRYV(dalloc(&b->op_id, b->n_ops));
    PTX_TRYV(dalloc(&b->ref_a, b->n_ops));
    PTX_TRYV(dalloc(&b->ref_b, b->n_ops));
    PTX_TRYV(dalloc(&b->payload, b->n_ops));
    PTX_TRYV(dalloc(&b->action, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYV(dalloc(&b->mark_type, b->n_ops + PTX_BYTE_PAD));
    PTX_TRYV(dalloc(&b->side_a, b->n_ops));
    PTX_TRYV(dalloc(&b->side_b, b->n_ops));
    PTX_TRYV(dalloc(&b->log_hdr, (uint64_t)P));
    PTX_TRYV(dalloc(&b->chg_hdr, b->n_changes + PTX_ENV_PAD));
    PTX_TRYV(dalloc(&b->chg_env, (b->n_changes + PTX_ENV_PAD) * ES));
    if (base->chg_env_hi) PTX_TRYV(dalloc(&b->chg_env_hi, (b->n_changes + PTX_ENV_PAD) * ES));
    if (P && b->n_changes) {
        PtxSyncGatherArgs G = {base->op_id, base->ref_a, base->ref_b, base->payload, base->action, base->mark_type, base->side_a, base->side_b,
                               b->op_id, b->ref_a, b->ref_b, b->payload, b->action, b->mark_type, b->side_a, b->side_b,
                               b->chg_hdr, b->chg_env, b->chg_env_hi, b->log_off, b->chg_off};
        hipLaunchKernelGGL(ptx_sync_gather_kernel, dim3(P), dim3(PTX_SYNC_GATHER_THREADS), 0, ctx->stream, A, G);
        PTX_TRYV(hipGetLastError());
    }
    PTX_TRYV(hipStreamSynchronize(ctx->stream));
#undef PTX_TRYV
    drop();
    const ptx_status st = census_and_shape(ctx, b, false);
    if (st != PTX_OK) {
        ptx_batch_free(ctx, b);
        return st;
    }
    *out = b;
    return PTX_OK;
}

struct ptx_host_batch_store {
    std::vector<uint64_t> log_off, op_id, ref_a, ref_b, chg_off;
    std::vector<uint32_t> payload, chg_hdr;
    std::vector<uint16_t> chg_env, chg_env_hi;
    std::vector<uint8_t> action, mark_type, side_a, side_b;
    std::vector<ptx_log_hdr> hdr;
};
void ptx_host_batch_free(ptx_host_batch* hb) {
    if (!hb) return;
    delete (ptx_host_batch_store*)hb->owner;
    memset(hb, 0, sizeof(*hb));
}
ptx_status ptx_batch_download(ptx_ctx* ctx, const ptx_dbatch* b, ptx_host_batch* out) {
    if (!ctx || !b || !out) return PTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    PTX_HIP(ctx, ptx_enter(ctx));
    ptx_host_batch_store* s = new ptx_host_batch_store();
    const uint64_t T = b->n_ops, L = b->n_logs, NC = b->chg_off ? b->n_changes : 0;
    s->log_off.resize(L + 1);
    s->op_id.resize(std::max<uint64_t>(T, 1));
    s->ref_a.resize(std::max<uint64_t>(T, 1));
    s->ref_b.resize(std::max<uint64_t>(T, 1));
    s->payload.resize(std::max<uint64_t>(T, 1));
    s->action.resize(std::max<uint64_t>(T, 1));
    s->mark_type.resize(std::max<uint64_t>(T, 1));
    s->side_a.resize(std::max<uint64_t>(T, 1));
    s->side_b.resize(std::max<uint64_t>(T, 1));
    s->hdr.resize(std::max<uint64_t>(L, 1));
    /* A small batch — the Change an editor's change() has just made: a few rows in fourteen arrays — comes back as ONE copy: the columns are gathered into the
     * context's staging block on the device and read from its pinned twin (fourteen copies into pageable memory were 0.19 ms of a 0.54 ms resident edit). */
    const uint64_t ES0 = PTX_ENV_STRIDE(b->max_actors);
    const size_t worst = (size_t)((L + 1) * 16 + T * 32 + L * sizeof(ptx_log_hdr) + NC * (4 + 4 * ES0) + 16 * 16);
    const bool packed = worst <= (256u << 10);
    struct Piece {
        void* dst;
        size_t at, bytes;
    };
    std::vector<Piece> pieces;
    size_t at = 0;
    hipError_t e = hipSuccess;
    if (packed) {
        if (ctx->stage_h_cap < worst) {
            if (ctx->stage_h) (void)hipHostFree(ctx->stage_h);
            ctx->stage_h = nullptr;
            ctx->stage_h_cap = 0;
            e = hipHostMalloc((void**)&ctx->stage_h, worst * 2, hipHostMallocDefault);
            if (e == hipSuccess) ctx->stage_h_cap = worst * 2;
        }
        if (e == hipSuccess && ctx->stage_d_cap < worst) {
            if (ctx->stage_d) (void)ptx_dev_free(ctx->stage_d);
            ctx->stage_d = nullptr;
            ctx->stage_d_cap = 0;
            e = ptx_dev_malloc((void**)&ctx->stage_d, worst * 2);
            if (e == hipSuccess) ctx->stage_d_cap = worst * 2;
        }
    }
    auto dl = [&](void* dst, const void* src, size_t bytes) {
        if (e != hipSuccess || !bytes) return;
        if (packed) {
            e = hipMemcpyAsync(ctx->stage_d + at, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
            pieces.push_back(Piece{dst, at, bytes});
            at += (bytes + 15) & ~(size_t)15;
        } else {
            e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
        }
    };
    dl(s->log_off.data(), b->log_off, (L + 1) * 8);
    dl(s->op_id.data(), b->op_id, T * 8);
    dl(s->ref_a.data(), b->ref_a, T * 8);
    dl(s->ref_b.data(), b->ref_b, T * 8);
    dl(s->payload.data(), b->payload, T * 4);
    dl(s->action.data(), b->action, T);
    dl(s->mark_type.data(), b->mark_type, T);
    dl(s->side_a.data(), b->side_a, T);
    dl(s->side_b.data(), b->side_b, T);
    dl(s->hdr.data(), b->log_hdr, L * sizeof(ptx_log_hdr));
    if (b->chg_off) {
        s->chg_off.resize(L + 1);
        const uint64_t ES = PTX_ENV_STRIDE(b->max_actors);
        s->chg_hdr.resize(std::max<uint64_t>(NC, 1));
        s->chg_env.resize(std::max<uint64_t>(NC * ES, 1));
        dl(s->chg_off.data(), b->chg_off, (L + 1) * 8);
        dl(s->chg_hdr.data(), b->chg_hdr, NC * 4);
        dl(s->chg_env.data(), b->chg_env, NC * ES * 2);
        if (b->chg_env_hi) {
            s->chg_env_hi.resize(std::max<uint64_t>(NC * ES, 1));
            dl(s->chg_env_hi.data(), b->chg_env_hi, NC * ES * 2);
        }
    }
    if (e == hipSuccess && packed && at) e = hipMemcpyAsync(ctx->stage_h, ctx->stage_d, at, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        delete s;
        return fail(ctx, PTX_ERR_HIP, std::string("batch download: ") + hipGetErrorString(e));
    }
    for (const Piece& q : pieces) memcpy(q.dst, ctx->stage_h + q.at, q.bytes);
    ptx_batch& h = out->b;
    h.n_logs = b->n_logs;
    h.n_ops = T;
    h.log_off = s->log_off.data();
    h.op_id = s->op_id.data();
    h.ref_a = s->ref_a.data();
    h.ref_b = s->ref_b.data();
    h.payload = s->payload.data();
    h.action = s->action.data();
    h.mark_type = s->mark_type.data();
    h.side_a = s->side_a.data();
    h.side_b = s->side_b.data();
    h.log_hdr = s->hdr.data();
    if (b->chg_off) {
        h.chg_off = s->chg_off.data();
        h.chg_hdr = s->chg_hdr.data();
        h.chg_env = s->chg_env.data();
        h.chg_env_hi = b->chg_env_hi ? s->chg_env_hi.data() : nullptr;
        h.max_actors = b->max_actors;
    }
    out->owner = s;
    return PTX_OK;
}

} /* extern "C" */
