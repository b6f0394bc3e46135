/*
 * peritext_hip.h — C ABI of the MI355X (gfx950) batch CRDT merge engine for Peritext's hot path.
 *
 * The reference (inkandswitch/peritext) has no FFI: its boundary is the TypeScript module API
 *     Micromerge.applyChange(change)            reference/src/micromerge.ts:499
 *     Micromerge.getTextWithFormatting(path)    reference/src/micromerge.ts:516 -> src/peritext.ts:337
 * called per replica by bridge.ts:253/288 and by the test harness (test/micromerge.ts:54-79,
 * test/fuzz.ts:198-205).  This header is what an N-API addon binds instead (INTEGRATION.md shows the
 * stub): ONE call applies MANY replica op logs and materialises the formatted documents.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types; every function returns a ptx_status
 *     (0 = ok) except the accessors; the last failure text is kept per context (ptx_last_error).
 *   - a context owns one HIP stream and every device allocation made through it; contexts are
 *     independent, one context must not be used from two threads at once.
 *   - per-LOG failures (the reference's throw sites, micromerge.ts:503,:507,:752) do not abort the
 *     batch: they are reported in ptx_log_result.status and that log's outputs are empty.
 *
 * Wire format of the op log (SoA, 32 bytes per op)
 *   A batch holds n_logs replica-logs.  A replica-log is the sequence of internal Operations
 *   (Change.ops flattened, micromerge.ts:60-71,:204-212) one replica applied, IN ITS APPLICATION
 *   ORDER.  Ops of log l are rows log_off[l] .. log_off[l+1]-1 of nine columns:
 *     op_id   u64  (counter << 32) | actorRank     "counter@actor" (micromerge.ts:488); actorRank =
 *                  rank of the actor string in UTF-16 code-unit order among the doc's actors, which
 *                  makes integer order == compareOpIds order (micromerge.ts:812-827)
 *     ref_a   u64  insert: elemId it was inserted after, 0 = HEAD (:153, :348); delete: elemId (:165);
 *                  mark: start.elemId (peritext.ts:17-21,:28)
 *     ref_b   u64  mark: end.elemId (peritext.ts:30); otherwise 0
 *     payload u32  insert: value id (index into the caller's string table); addMark link: url id;
 *                  add/removeMark comment: DOC-LOCAL comment id (rank among the document's comment ids, shared by
 *                  all replicas of the document) whose numeric order equals the code-unit order of the id strings
 *                  (peritext.ts:318 keeps the array sorted by id)
 *     action  u8   PTX_ACT_*      mark_type u8  PTX_MARK_* (schema.ts:125 ALL_MARKS order)
 *     side_a  u8   PTX_SIDE_* of start        side_b u8  PTX_SIDE_* of end
 *   Ops on the map objects (set / del / makeMap on the root map or a nested map) are PTX_ACT_MAPSET / PTX_ACT_MAPDEL rows: the text path
 *   ignores them, ptx_root_map resolves them; anything else is PTX_ACT_NOP.
 *
 * Output (all per log, canonical — two replicas have deep-equal getTextWithFormatting output iff
 * their canonical outputs, and therefore their digests, are equal):
 *     values     u32[n_visible]   value ids of the visible elements in document order
 *     spans      {start, attr}[n_spans]   maximal runs of visible elements with equal marks
 *                (peritext.ts:438-455): start = visible index of the first element, attr = flags<<28 | link url id
 *     cintervals {id, start, end}[n_cintervals]  for every comment id the maximal visible ranges
 *                [start,end) on which that comment is present, sorted by (id, start).  A span's
 *                `comment` array is the set of ids whose interval covers it (present iff
 *                PTX_ATTR_COMMENT is set — `comment: []` is a real state).
 *     digest     2 x u64 multiset hash of the above (peritext_amd/canon.py restates it).  Compared only with digests of the SAME build of the library
 *                (replicas of a document, ranks of a job): the per-item mixing function is not part of the ABI (round 6 replaced it, csrc/merge_core.h)
 *   Output rows of log l start at row log_off[l] of each output array (a log never produces more
 *   rows than it has ops), so no cross-log compaction or device-side allocation is needed.
 */
#ifndef PERITEXT_HIP_H
#define PERITEXT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTX_ABI_VERSION 7u

/* Operation.action (micromerge.ts:150-212, peritext.ts:25-65) */
enum {
    PTX_ACT_MAKELIST = 0,   /* creates the text list; exactly one per log, ignored by the kernels */
    PTX_ACT_INSERT = 1,     /* {action:"set", insert:true}  -> applyListInsert  micromerge.ts:614 */
    PTX_ACT_DELETE = 2,     /* {action:"del", elemId}       -> applyListUpdate  micromerge.ts:677 */
    PTX_ACT_ADDMARK = 3,    /* applyAddRemoveMark peritext.ts:154 */
    PTX_ACT_REMOVEMARK = 4,
    PTX_ACT_NOP = 5,        /* an op the engine does not model: no effect */
    /* ops on MAP objects (the root map or a nested map), micromerge.ts:572-602: last-writer-wins per (object, key).  No effect on the
     * text path (ptx_merge ignores them); ptx_root_map resolves them.  ref_a = the map's object id (0 = the root map, else the opId
     * of the makeMap that created it), ref_b = key id (batch-wide string table).  The text list's own PTX_ACT_MAKELIST row is such a
     * write too (root map, its key in ref_b, kind PTX_MAPV_LIST). */
    PTX_ACT_MAPSET = 6,     /* {action:"set", key, value} / makeMap / makeList: mark_type = PTX_MAPV_*, payload = value id (scalars) */
    PTX_ACT_MAPDEL = 7      /* {action:"del", key} */
};
/* what a PTX_ACT_MAPSET row writes (its mark_type byte) / what ptx_root_entry.kind says */
enum { PTX_MAPV_SCALAR = 0, PTX_MAPV_MAP = 1, PTX_MAPV_LIST = 2, PTX_MAPV_DELETED = 3 };

/* markType, in ALL_MARKS order (schema.ts:125) */
enum { PTX_MARK_STRONG = 0, PTX_MARK_EM = 1, PTX_MARK_COMMENT = 2, PTX_MARK_LINK = 3 };

/* BoundaryPosition.type (peritext.ts:17-21) */
enum { PTX_SIDE_BEFORE = 0, PTX_SIDE_AFTER = 1, PTX_SIDE_START_OF_TEXT = 2, PTX_SIDE_END_OF_TEXT = 3 };

/* span attr: flags in the top 4 bits, link url id in the low 28 (0 when no link) */
#define PTX_ATTR_STRONG 0x10000000u
#define PTX_ATTR_EM 0x20000000u
#define PTX_ATTR_LINK 0x40000000u
#define PTX_ATTR_COMMENT 0x80000000u /* key `comment` present (possibly []) */
#define PTX_ATTR_ID_MASK 0x0fffffffu

/* Change envelope: chg_hdr word and chg_env row stride (u16 entries, a multiple of 4 so that rows are 8-byte aligned) */
#define PTX_CHG_ACTOR_SHIFT 20u
#define PTX_CHG_NOPS 0x000FFFFFu
#define PTX_ENV_STRIDE(max_actors) ((1u + (uint32_t)(max_actors) + 3u) & ~3u)
#define PTX_ENV_SATURATED 65535u

/* elem_rank: bit 31 marks a tombstone, the low 31 bits are the document position */
#define PTX_RANK_TOMBSTONE 0x80000000u
#define PTX_RANK_MASK 0x7fffffffu

typedef int32_t ptx_status;
enum {
    PTX_OK = 0,
    /* per-log (ptx_log_result.status): mirror the reference's throw sites */
    PTX_ERR_ELEM_NOT_FOUND = 1,  /* RangeError "List element not found"      micromerge.ts:752 */
    PTX_ERR_SEQ_GAP = 2,         /* RangeError "Expected sequence number"    micromerge.ts:503 */
    PTX_ERR_MISSING_DEP = 3,     /* RangeError "Missing dependency"          micromerge.ts:507 */
    PTX_ERR_DUPLICATE_OP = 4,    /* same opId twice in one log (the seq check makes this impossible upstream) */
    PTX_ERR_CAPACITY = 5,        /* log beyond what this build holds (ptx_merge: beyond the HBM-staged path's bounds or a forced LDS window; the on-chip-only entry points: beyond one CU's LDS) */
    PTX_ERR_BAD_OP = 6,          /* malformed row: unknown action / mark type / comment id beyond the header's n_comment_ids */
    PTX_ERR_INDEX_OOB = 7,       /* RangeError "List index out of bounds"    micromerge.ts:804 (ptx_change only) */
    /* per-pair (ptx_sync_replicas only) */
    PTX_ERR_SYNC_NOT_CONVERGED = 8, /* "applyChanges did not converge"       test/merge.ts:18-19: more attempts than max_attempts, or a pass that admits nothing */
    /* call-level */
    PTX_ERR_INVALID_ARG = 100,
    PTX_ERR_HIP = 101,           /* a HIP runtime call failed; see ptx_last_error */
    PTX_ERR_NO_DEVICE = 102,
    PTX_ERR_OOM = 103
};

/* Per-log census, part of the wire format: it lets the kernel size its on-chip lists and id bitmaps
 * before it has seen a row, so the op columns are streamed ONCE.  The encoder that flattens Change.ops
 * (micromerge.ts:60-71) knows these numbers for free.  The kernel verifies them against the rows
 * (a wrong header is PTX_ERR_BAD_OP, never a wrong result); a batch may omit them (log_hdr = NULL),
 * then the library computes them with a small pre-pass kernel when the batch becomes resident. */
typedef struct ptx_log_hdr {
    uint32_t n_ins;       /* PTX_ACT_INSERT rows */
    uint32_t n_del;       /* PTX_ACT_DELETE rows */
    uint32_t n_mark[4];   /* add/removeMark rows per PTX_MARK_* */
    uint32_t max_counter; /* largest counter of any op_id of the log */
    uint32_t max_actor;   /* largest actorRank of any op_id of the log */
    uint32_t n_comment_ids; /* comment payloads of the log are < n_comment_ids: largest doc-local comment id the log uses + 1
                               (0 without comment ops).  Comment ids are ranks over ALL replicas of the document, so a replica
                               that has seen only some of the comments still carries the document's ranks (an upper bound
                               is accepted: it only sizes the per-id tables) */
    uint32_t reserved;
} ptx_log_hdr;

/* One batch of replica-logs.  All pointers are HOST pointers for ptx_batch_upload /
 * ptx_apply_materialize and DEVICE pointers for ptx_batch_wrap_device. */
typedef struct ptx_batch {
    uint32_t n_logs;
    uint32_t reserved;
    uint64_t n_ops;            /* == log_off[n_logs] */
    const uint64_t* log_off;   /* [n_logs + 1] */
    const uint64_t* op_id;     /* [n_ops] */
    const uint64_t* ref_a;     /* [n_ops] */
    const uint64_t* ref_b;     /* [n_ops] */
    const uint32_t* payload;   /* [n_ops] */
    const uint8_t* action;     /* [n_ops] */
    const uint8_t* mark_type;  /* [n_ops] */
    const uint8_t* side_a;     /* [n_ops] */
    const uint8_t* side_b;     /* [n_ops] */
    /* optional causal envelope (Change headers, micromerge.ts:60-71); NULL = skip causal admission.
     * When present (host batches: ptx_batch_upload / ptx_apply_materialize) the kernel admits every change
     * exactly like applyChange (micromerge.ts:499-511): seq == clock[actor] + 1 (PTX_ERR_SEQ_GAP) and
     * clock[a] >= deps[a] for all a (PTX_ERR_MISSING_DEP); 4 + 2 * PTX_ENV_STRIDE(max_actors) extra bytes are read per
     * change (12 B up to three actors).  chg_off[l]..chg_off[l+1]-1 are the changes of log l in application order. */
    const uint64_t* chg_off;   /* [n_logs + 1] or NULL */
    const uint32_t* chg_hdr;   /* [n_changes] actorRank << PTX_CHG_ACTOR_SHIFT | ops in the change (consecutive rows of the log) */
    const uint16_t* chg_env;   /* [n_changes * PTX_ENV_STRIDE(max_actors)] one row per change: seq, deps[0 .. max_actors) (0 = none),
                                  zero padding.  The LOW 16 bits of every value when the batch carries chg_env_hi; without it the
                                  values themselves, saturated at 65 535 (PTX_ENV_SATURATED) — a log of up to 65 533 changes can
                                  never admit such a change: the reference's RangeError either way (micromerge.ts:501-509) */
    uint32_t max_actors;       /* actors of a document (deps entries per change) */
    uint32_t reserved2;
    const ptx_log_hdr* log_hdr; /* [n_logs] or NULL (the library computes it) */
    /* optional wide envelope (ABI 6): the HIGH 16 bits of every chg_env value, same shape; NULL = every seq / dep of the batch fits 16
     * bits.  seq / deps are plain numbers in the reference (micromerge.ts:499-511): a replica that typed one change per keystroke
     * (bridge.ts:535) passes 65 535 changes of one actor.  Encoders emit the column whenever some value of the batch exceeds 65 534;
     * values are then EXACT (lo | hi << 16, no saturation).  A log whose rows of it are not all zero, or that holds more than 65 533
     * changes, is merged by the HBM-staged kernel (32-bit admission table); a log of more than 65 533 changes in a batch WITHOUT the
     * column cannot be represented and reports PTX_ERR_CAPACITY — never a spurious PTX_ERR_SEQ_GAP. */
    const uint16_t* chg_env_hi; /* [n_changes * PTX_ENV_STRIDE(max_actors)] or NULL */
} ptx_batch;

typedef struct ptx_span {
    uint32_t start; /* visible index of the first element of the span */
    uint32_t attr;  /* PTX_ATTR_* | link url id */
} ptx_span;

typedef struct ptx_cinterval {
    uint32_t id;    /* doc-local comment id */
    uint32_t start; /* visible index, inclusive */
    uint32_t end;   /* visible index, exclusive */
} ptx_cinterval;

typedef struct ptx_log_result {
    uint32_t status;        /* PTX_OK or a per-log PTX_ERR_* */
    uint32_t n_ops;         /* ops applied (the makeList and NOP rows excluded) */
    uint32_t n_elems;       /* list elements incl. tombstones */
    uint32_t n_visible;     /* rows of `values` */
    uint32_t n_spans;       /* rows of `spans` */
    uint32_t n_cintervals;  /* rows of `cintervals` */
    uint32_t reserved[2];   /* [0] diagnostic: LDS bytes the log needed; [1] on a per-row failure (status 1-4, 6): the row of the log at
                               which the reference's sequential replay would have thrown (the first op of the change for seq / deps
                               failures), else 0xffffffff */
    uint64_t digest[2];
} ptx_log_result;

/* Host-side view of a result set (returned by ptx_result_download[_range] / ptx_apply_materialize).  ABI 7: the rows are COMPACT — only the rows that
 * exist come down (a 4 096-op fuzz log shows a few dozen characters; round 4 downloaded one row per op: 2.4 GB for 100 M ops whose output is ~1 MB) —
 * gathered on the device into dense arrays and copied into pinned host memory:
 *     values[value_off[l] .. value_off[l + 1])          the n_visible value ids of log l, in document order
 *     spans[span_off[l] .. span_off[l + 1])             its n_spans span rows
 *     cintervals[cint_off[l] .. cint_off[l + 1])        its n_cintervals comment-interval rows
 * (a failed log has none).  elem_rank, where the context produces it, keeps one entry per op ROW of the downloaded logs (row r of log l at
 * log_off[l] - log_off[first log] + r).  Owned by the library until ptx_result_free. */
typedef struct ptx_result {
    uint32_t n_logs;
    uint32_t reserved;
    uint64_t n_rows;                  /* op rows of the downloaded logs (entries of elem_rank) */
    const ptx_log_result* logs;       /* [n_logs] */
    const uint32_t* values;           /* [value_off[n_logs]] */
    const ptx_span* spans;            /* [span_off[n_logs]] */
    const ptx_cinterval* cintervals;  /* [cint_off[n_logs]] */
    const uint32_t* elem_rank;        /* [n_rows] or NULL (PTX_FLAG_NO_ELEM_RANK).  Per op row: document position (incl. tombstones) of the
                                         element an INSERT row created (what findListElement(...).index
                                         would return, micromerge.ts:731), | PTX_RANK_TOMBSTONE when the
                                         element is deleted; 0xffffffff for other rows.  Enough to resolve
                                         cursors (getCursor / resolveCursor, micromerge.ts:465-477) on the host */
    const uint64_t* value_off;        /* [n_logs + 1] exclusive prefix sum of logs[].n_visible */
    const uint64_t* span_off;         /* [n_logs + 1] ... of logs[].n_spans */
    const uint64_t* cint_off;         /* [n_logs + 1] ... of logs[].n_cintervals */
    void* owner;
} ptx_result;

/* ---- incremental patch streams (what applyChange RETURNS, micromerge.ts:499 -> Patch[]) ----
 * One record per patch, in the replica's application order.  `row` = the op row of the log that produced it.
 *   PTX_PATCH_MAKELIST        the makeList op itself                          micromerge.ts:575
 *   PTX_PATCH_INSERT          a = visible index, b = marks of the new char (PTX_ATTR_* | link url id, as ptx_span.attr;
 *                             PTX_ATTR_COMMENT = key `comment` present)       micromerge.ts:661-671, peritext.ts:328
 *   PTX_PATCH_INSERT_COMMENT  follows its INSERT record: a = one doc-local comment id of the new char's marks
 *                             (ids in no particular order; the reference lists them sorted by id string)
 *   PTX_PATCH_DELETE          a = visible index, b = count (1)                micromerge.ts:696-703
 *   PTX_PATCH_ADDMARK / PTX_PATCH_REMOVEMARK  a = startIndex, b = endIndex (visible, exclusive); markType and attrs
 *                             are those of op `row`                           peritext.ts:251-281 */
enum { PTX_PATCH_MAKELIST = 0, PTX_PATCH_INSERT = 1, PTX_PATCH_DELETE = 2, PTX_PATCH_ADDMARK = 3, PTX_PATCH_REMOVEMARK = 4, PTX_PATCH_INSERT_COMMENT = 5 };
typedef struct ptx_patch {
    uint32_t row;
    uint32_t kind; /* PTX_PATCH_* */
    uint32_t a;
    uint32_t b;
} ptx_patch;
typedef struct ptx_patch_log {
    uint32_t status;    /* PTX_OK, or the log's merge status (no stream for a log the reference would have thrown on),
                           or PTX_ERR_CAPACITY (more records than the room for them: n_patches is then the exact count; a log beyond the bounds of the
                           replay: 2^26 - 1 list elements, 65 534 comment ops, 65 535 comment ids) */
    uint32_t n_patches; /* records of this log */
} ptx_patch_log;
/* Host-side view of the patch streams of a batch: records of log l at patches[patch_off[l] .. patch_off[l] + logs[l].n_patches).
 * Owned by the library until ptx_patches_free. */
typedef struct ptx_patches {
    uint32_t n_logs;
    uint32_t launches;          /* launches of the replay kernel it took: 1 (a log that outgrows the guessed capacity continues in an overflow extent; the records are
                                   packed to exact offsets on the device); 2 only when the overflow arena itself ran out */
    float kernel_ms;            /* duration of the last replay (HIP events): the launch of the logs whose state fits the LDS and the HBM-state launch together */
    uint32_t reserved;          /* hbm_logs: the logs the HBM-state kernel replayed (their replay state beyond one CU's LDS, or PTX_FLAG_REPLAY_HBM_STATE) */
    const uint64_t* patch_off;  /* [n_logs + 1] */
    const ptx_patch_log* logs;  /* [n_logs] */
    const ptx_patch* patches;   /* [patch_off[n_logs]] */
    void* owner;
} ptx_patches;

typedef struct ptx_ctx ptx_ctx;          /* device context: stream + allocations */
typedef struct ptx_dbatch ptx_dbatch;    /* a batch resident in HBM */
typedef struct ptx_dresult ptx_dresult;  /* result buffers resident in HBM */

/* ptx_create flags */
#define PTX_FLAG_NO_ELEM_RANK 1u /* do not produce ptx_result.elem_rank (saves 4 B/op of HBM writes) */
#define PTX_FLAG_NO_ADMISSION 2u /* ignore the Change envelope (chg_*) even when the batch carries it: no seq / deps checks */
#define PTX_FLAG_REPLAY_LDS_ONLY 8u /* ptx_replay_patches keeps its whole working set in LDS even where it exceeds 5.5 KB per log (by default the per-slot link urls and the
                                      tables of applied ops then live in global memory: four times the logs per CU); tuning / A-B */
#define PTX_FLAG_REPLAY_HBM_STATE 16u /* ptx_replay_patches replays EVERY log with its state in global scratch (by default only the logs whose state does not fit one
                                         CU's LDS: that kernel pays a trip to the L2 per state access); tests / measurement */
#define PTX_FLAG_ACCUM_HBM_STATE 32u /* ptx_accumulate_patches / ptx_check_patches accumulate EVERY log with its state in global scratch (by default only the logs whose
                                        state does not fit one CU's LDS); tests / measurement */
#define PTX_FLAG_PAD_GATHER 4u   /* ptx_allgather_digests always takes its padded path (pack, all-gather of max(counts) pairs per rank, compact on the
                                    device) even when every rank holds the same number of logs: same result; lets a one-GPU host exercise that path */
#define PTX_FLAG_READMIT 64u     /* ptx_merge walks the Change envelope of every log in EVERY launch, as the library did before it kept admission marks, and leaves
                                    the marks of the batch alone.  By default a resident batch remembers, per log, the prefix of changes whose seq / deps checks
                                    passed in an earlier launch of any context (its columns never change, so they pass again) and a launch walks only the changes
                                    behind it: none for a batch merged before, the appended ones for a batch grown by ptx_batch_append[_device].  Results are the
                                    same either way; a log that fails is walked and reported again in every launch.  The same holds for the ROW INDEX of the
                                    batch (ptx_merge below): a launch of such a context neither writes nor reads it and classifies every row — "a launch as
                                    the library did before it remembered anything", i.e. what a batch's first merge costs, at will.  The diagnostic launches
                                    (ptx_merge_phase_cycles) stay out of both as well.  For measurement and tests */

/* ---- lifecycle ---- */
uint32_t ptx_abi_version(void);
/* device_ordinal: HIP device index.  Fails with PTX_ERR_NO_DEVICE when no gfx950 GPU is visible:
 * there is NO CPU fallback behind this ABI. */
ptx_status ptx_create(int device_ordinal, uint32_t flags, ptx_ctx** out);
void ptx_destroy(ptx_ctx* ctx);
/* Launch shape of the batches made resident AFTER this call (upload / append / generate / wrap): threads per replica log (a
 * multiple of 64, <= 1024) and the LDS window per log in bytes; 0 = the library's own choice by log size (the default).  A tuning
 * knob: results do not depend on it; a window too small for a log is that log's PTX_ERR_CAPACITY. */
ptx_status ptx_set_launch_shape(ptx_ctx* ctx, uint32_t threads_per_log, uint32_t lds_bytes_per_log);
const char* ptx_last_error(const ptx_ctx* ctx); /* ctx may be NULL: last ptx_create failure */

/* ---- the drop-in call: replaces a loop of applyChange(...) + getTextWithFormatting(["text"]) ---- */
/* Upload `batch` (host pointers), run the merge, download the results, synchronise. */
ptx_status ptx_apply_materialize(ptx_ctx* ctx, const ptx_batch* batch, ptx_result* out);
void ptx_result_free(ptx_result* res);

/* ---- staged form (what bench.py and the multi-GPU driver use: inputs resident in HBM) ---- */
ptx_status ptx_batch_upload(ptx_ctx* ctx, const ptx_batch* host, ptx_dbatch** out);
/* Build a resident batch made of `copies` back-to-back copies of `host` (distinct HBM addresses,
 * used to scale a synthetic batch to BASELINE sizes without regenerating it). */
ptx_status ptx_batch_upload_tiled(ptx_ctx* ctx, const ptx_batch* host, uint32_t copies, ptx_dbatch** out);
/* Adopt caller-owned DEVICE pointers (e.g. torch tensors' data_ptr); nothing is copied or freed.  (The caller may rewrite that memory between merges: such a
 * batch keeps no admission marks, see ptx_merge.) */
ptx_status ptx_batch_wrap_device(ptx_ctx* ctx, const ptx_batch* device, ptx_dbatch** out);
/* Streaming append: a NEW resident batch whose log l = log l of `base` followed by log l of `more` (host
 * pointers; the changes that arrived since, in application order; same n_logs, empty logs allowed).  Rows are copied
 * device to device; `base` stays valid.  `more` must be encoded with the tables of `base` (actor ranks, comment ranks,
 * value / url ids); both batches carry the Change envelope with the same max_actors, or neither does. */
ptx_status ptx_batch_append(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_batch* more, ptx_dbatch** out);
void ptx_batch_free(ptx_ctx* ctx, ptx_dbatch* b);
uint32_t ptx_batch_n_logs(const ptx_dbatch* b);
uint64_t ptx_batch_n_ops(const ptx_dbatch* b);
uint64_t ptx_batch_n_changes(const ptx_dbatch* b); /* rows of the Change envelope (0 = the batch has none) */
uint32_t ptx_batch_max_actors(const ptx_dbatch* b); /* actor ranks per envelope row: the width of a ptx_batch_at_versions clock (0 = the batch has no envelope) */
/* Launch shape the library derived from the batch's log headers: threads per workgroup (= per log) and
 * dynamic LDS bytes per workgroup (the largest log's working set; it sets how many logs share a CU).  When at most a
 * tenth of the logs need more LDS than would let one more log share a CU, those are merged in a second launch of
 * their own and the figure reported here is that of the main launch. */
void ptx_batch_launch_shape(const ptx_dbatch* b, uint32_t* threads, uint32_t* lds_bytes);

ptx_status ptx_result_alloc(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult** out);
void ptx_dresult_free(ptx_ctx* ctx, ptx_dresult* r);

/* Enqueue the merge of every log of `b` on the context's stream (asynchronous).
 * Causal admission is kept, not repeated: a batch the library made with the Change envelope (upload, append, generate, ptx_change, ptx_sync_replicas — not
 * ptx_batch_wrap_device, whose memory is the caller's) carries one 16-byte ADMISSION MARK per log on the device — {changes admitted, their rows, the vector clock
 * after them} — written by the first launch in which all of the log's changes pass applyChange's seq / deps checks (micromerge.ts:499-511: the reference, too,
 * checks a change once, when it arrives, against a clock that is replica state).  A later launch of ANY context on that batch reads the mark instead of the
 * envelope; ptx_batch_append[_device] hands the marks of `base` to the grown batch (documents of up to three actors), whose next launch checks the appended
 * changes only.  A log that fails writes no mark: it is walked, and fails with the same status and row, in every launch.  Results never depend on the marks
 * (PTX_FLAG_READMIT: ignore them); launches on several streams may share a batch — a mark is one aligned 16-byte store, and every value a launch can read
 * there is true.
 * The rows are classified once, too: a batch that owns its columns and whose logs all have 16-bit id keys carries a ROW INDEX on the device (about 4.1 bytes per
 * row) — per log the lists the row pass derives from op_id / action / mark_type and the header: the inserts, the deletes, the mark ops by type as
 * `row | id key << 16`, and the add / remove bitmap.  The FIRST eligible ptx_merge of the batch writes it, for every log that passes the row pass's checks
 * (census against the header, malformed rows, repeated op ids), and records an event behind its launches; a later ptx_merge reads it instead of the rows if it
 * is ordered after that whole launch — on the writer's stream by stream order, on another stream once the event has completed (until then such a merge simply
 * classifies its rows as before: nothing waits).  A log that fails a check is never indexed and fails with the same status and row in every launch.  A batch
 * made by ptx_batch_append[_device] starts with an empty index of its own.  No index: ptx_batch_wrap_device, ptx_apply_materialize (merged once), batches
 * with a wide-key log, the logs beyond one CU's LDS, and a batch whose index could not be allocated (no error).
 * The marks and the index are the TWO things a merge writes into a batch; a batch's columns stay immutable, and results never depend on either. */
ptx_status ptx_merge(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r);
/* Same, `iters` times back to back, bracketed by HIP events on the context's stream:
 * *ms_total = elapsed milliseconds of the `iters` launches (for roofline accounting). */
ptx_status ptx_merge_timed(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r, uint32_t iters, float* ms_total);
/* Diagnostic: run the merge once with per-phase cycle stamps (thread 0 of every workgroup) and return
 * the shader-clock cycles summed over all workgroups per phase: cycles[k], k < n <= 16, phases in the
 * order of merge_core.h (P1 classify, P2 index, P3a buckets, P3b child order, P3c tour+ranking, P4
 * tombstones, P5a values+mark intervals, P5b LWW, P5c comments, P6 spans).  Not for timed runs. */
ptx_status ptx_merge_phase_cycles(ptx_ctx* ctx, const ptx_dbatch* b, ptx_dresult* r, uint64_t* cycles, uint32_t n);
/* Diagnostic (profiling runs only): stream every op column — and the Change envelope when the batch has one — exactly once
 * with the element widths the merge kernel uses (kernel `ptx_calib_stream_kernel`); *bytes_read = the bytes that stream is,
 * 32 per op row + the envelope.  It calibrates the HBM-traffic PMC counters on a known byte count in this library's own
 * access pattern (tools/pmc_traffic.sh).  Synchronises. */
ptx_status ptx_calib_stream(ptx_ctx* ctx, const ptx_dbatch* b, uint64_t* bytes_read);
ptx_status ptx_sync(ptx_ctx* ctx);
/* Run the context's launches and copies on the caller's HIP stream (e.g. torch's current stream: everything stays
 * stream-ordered with the caller's own kernels and no host-side synchronisation is needed between them).  `hip_stream`
 * = a hipStream_t; NULL returns to the context's own stream.  The stream stays the caller's. */
ptx_status ptx_set_stream(ptx_ctx* ctx, void* hip_stream);
/* Documents whose `replicas` consecutive logs all have the same digest (= converged, test/fuzz.ts:277-278), counted on the
 * device: *count_device (a u64 in DEVICE memory) is overwritten.  n_logs must be a multiple of `replicas`. */
ptx_status ptx_count_converged(ptx_ctx* ctx, const ptx_dresult* r, uint32_t replicas, uint64_t* count_device);

ptx_status ptx_result_download(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, ptx_result* out);
/* The same for the logs [first_log, first_log + n_logs) only (e.g. a sample of a large resident batch): out->n_logs = n_logs,
 * out->n_rows = their rows, row r of the k-th log of the range at index (log_off[first_log + k] - log_off[first_log]) + r. */
ptx_status ptx_result_download_range(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, uint32_t first_log, uint32_t n_logs, ptx_result* out);
/* Only the per-log rows (status, counts, digests): [n_logs] ptx_log_result into caller memory. */
ptx_status ptx_result_download_logs(ptx_ctx* ctx, const ptx_dresult* r, ptx_log_result* out, uint32_t n_logs);
/* Device address of the per-log result rows (for a collective on the digests); never freed by the caller. */
const ptx_log_result* ptx_dresult_logs_device(const ptx_dresult* r);
/* Pack the digests of logs [first, first+count) as 2*count u64 into DEVICE memory `dst`
 * (e.g. a torch tensor that is then all-gathered with RCCL), on the context's stream. */
ptx_status ptx_pack_digests(ptx_ctx* ctx, const ptx_dresult* r, uint32_t first, uint32_t count, uint64_t* dst_device);

/* ---- multi-GPU: the digest all-gather (the reference's convergence assert, test/fuzz.ts:277-278, for a sharded batch) ----
 * Documents shard across ranks (one process per GPU), every replica of a document on one rank; the only exchange is an
 * all-gather of the per-replica 128-bit digests over RCCL (xGMI inside a node) so that every rank can state global convergence.
 * RCCL is loaded at run time (librccl.so.1) by the first of these calls: a single-GPU host never needs it. */
#define PTX_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct ptx_comm ptx_comm;
/* Optional, before the first ptx_comm_* call of the process: bind the collective library (the five RCCL entry points this ABI uses) from `path`
 * instead of the process's librccl.so.1 — a host that ships its own RCCL build; the test-suite's shared-memory stand-in, which lets several ranks
 * share one GPU.  PTX_ERR_INVALID_ARG once a library is bound. */
ptx_status ptx_comm_use_library(ptx_ctx* ctx, const char* path);
/* Rank 0 makes the id (ncclGetUniqueId) and hands it to the other ranks over the host's own channel. */
ptx_status ptx_comm_unique_id(ptx_ctx* ctx, uint8_t id[PTX_COMM_ID_BYTES]);
/* Collective over all ranks (ncclCommInitRank) on the context's device. */
ptx_status ptx_comm_init(ptx_ctx* ctx, const uint8_t id[PTX_COMM_ID_BYTES], uint32_t rank, uint32_t n_ranks, ptx_comm** out);
void ptx_comm_destroy(ptx_ctx* ctx, ptx_comm* comm);
uint32_t ptx_comm_n_ranks(const ptx_comm* comm); /* 0 for NULL: hosts check the length of `counts` against it */
uint32_t ptx_comm_rank(const ptx_comm* comm);
/* All-gather of the digests of every rank's result: counts[r] = replica logs of rank r (host array [n_ranks]; counts[rank] must be
 * the logs of `r`), out_device = [sum(counts)] x 2 u64 in DEVICE memory, rank-major.  Enqueued on the context's stream; ranks
 * whose blocks differ in size are gathered padded and compacted on the device. */
ptx_status ptx_allgather_digests(ptx_ctx* ctx, ptx_comm* comm, const ptx_dresult* r, const uint32_t* counts, uint64_t* out_device);
/* Documents whose `replicas` consecutive digest pairs are all equal, over a gathered digest array in DEVICE memory (n_logs pairs):
 * *count_device (a u64 in DEVICE memory) is overwritten.  A failed log has the digest {0, 0} and never converges with a good one;
 * per-log statuses stay with the rank that owns the log. */
ptx_status ptx_count_converged_digests(ptx_ctx* ctx, const uint64_t* digests_device, uint64_t n_logs, uint32_t replicas, uint64_t* count_device);

/* Device memory for hosts that have no HIP binding of their own (the N-API addon): scratch for out_device / count_device above.
 * ptx_device_read copies `bytes` back to the host after everything enqueued on the context's stream has completed. */
ptx_status ptx_device_alloc(ptx_ctx* ctx, uint64_t bytes, void** out_device);
void ptx_device_free(ptx_ctx* ctx, void* device);
ptx_status ptx_device_read(ptx_ctx* ctx, const void* device, void* host, uint64_t bytes);

/* ---- patch streams ---- */
/* Replay every log of `b` in application order and return the Patch[] stream each applyChange would have returned.
 * `r` must be the result of ptx_merge on the same batch, produced WITH elem_rank (no PTX_FLAG_NO_ELEM_RANK) and
 * complete (the call synchronises).  Capacity is guessed (2 records per op) and the launch repeated once with exact
 * sizes when a log produced more. */
ptx_status ptx_replay_patches(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, ptx_patches* out);
/* The same for the TAIL of every log: first_row[l] (host array [n_logs]; NULL = 0 everywhere) is the first row of log l whose records are wanted —
 * what the applyChange calls of the Changes appended since the last call return (a host that keeps its replicas resident: ptx_batch_append, ptx_merge,
 * this).  The rows before are replayed for their state only: no record of theirs is written, counted or downloaded; `row` in the records stays the row
 * in the log.  first_row[l] >= the log's rows: an empty stream. */
ptx_status ptx_replay_patches_from(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const uint32_t* first_row, ptx_patches* out);
void ptx_patches_free(ptx_patches* p);

/* ---- the consumer side: accumulatePatches (reference/test/accumulatePatches.ts; the fuzzer's third assertion, test/fuzz.ts:245-278) ----
 * A stream is applied record by record to a list of characters {value id, attr word, set of comment ids} that starts empty:
 *   PTX_PATCH_MAKELIST        nothing
 *   PTX_PATCH_INSERT          a character with value payload[row], attr b and no ids at index a; it is "the last inserted character"
 *   PTX_PATCH_INSERT_COMMENT  id a joins the last inserted character's set (legal only right behind an INSERT or another INSERT_COMMENT)
 *   PTX_PATCH_DELETE          b characters from index a go (a foreign stream may fold deletes: b > 1)
 *   PTX_PATCH_ADDMARK / PTX_PATCH_REMOVEMARK  characters [a, b), the type = mark_type[row]: strong / em set / clear the flag; link sets PTX_ATTR_LINK and
 *                             payload[row] / clears both; comment sets PTX_ATTR_COMMENT and adds id payload[row] / sets PTX_ATTR_COMMENT (the key stays, possibly
 *                             []) and discards THAT id only (the reference's checker drops the whole key; the replica itself does not, peritext.ts:318-320)
 * The result is the canonical form of the merge: values, a span wherever attr or the id set changes, one comment interval per id and maximal run, n_elems = the
 * INSERT records, and the digest the merge computes for those rows.  Per-log status: the stream's own when that is not PTX_OK (no rows, digest {0, 0});
 * PTX_ERR_INDEX_OOB (an insert index beyond the length, a delete that reaches past the end, a mark with b > length or a > b; a == b is an empty range);
 * PTX_ERR_BAD_OP (an unknown kind, row >= the log's rows, an INSERT_COMMENT behind anything else, a comment id >= the log header's n_comment_ids, a mark
 * record whose row is not a mark op); PTX_ERR_CAPACITY (more INSERT records than the log has insert rows, or more output rows than the log has rows).  A failed
 * log has no rows, reserved[1] = the index of its first bad record (0xffffffff otherwise); the other logs of the call are unaffected. */
/* host records of any origin (p->patch_off / logs / patches; p->n_logs == the batch's logs) -> canonical rows (elem_rank NULL); synchronises */
ptx_status ptx_accumulate_patches(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_patches* p, ptx_result* out);

typedef struct ptx_patch_check_log {
    uint32_t status;            /* as above */
    uint32_t agrees;            /* the stream's {n_elems, n_visible, n_spans, n_cintervals, digest} equal the merge's */
    uint32_t n_patches;         /* records of the log's stream */
    uint32_t first_bad_record;  /* 0xffffffff when status == PTX_OK */
    uint64_t digest[2];         /* of the accumulated stream */
} ptx_patch_check_log;
/* Replay every log of `b` (whole streams, as ptx_replay_patches) and accumulate the records ON THE DEVICE, where the replay wrote them: no record is downloaded.
 * `r` = ptx_merge of `b` WITH elem_rank, complete.  out: host [n_logs]; *n_disagree = the logs with status PTX_OK and agrees == 0.  Synchronises. */
ptx_status ptx_check_patches(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, ptx_patch_check_log* out, uint64_t* n_disagree);
/* Diagnostic: HIP-event durations of the last successful ptx_check_patches of the context (both 0 before the first).
 *   *replay_ms  the replay launches of the LAST replay attempt only (ptx_patches.kernel_ms): where the replay ran twice, because the record arena or a log's extent
 *               ran out, the first attempt's kernel time is not in it.
 *   *accum_ms   the accumulate launches, a SUM over the packed ranges (one range unless device memory is short or PTX_REPLAY_PACK_RECORDS is set); the
 *               pack kernel's time is in neither figure. */
ptx_status ptx_check_patches_ms(const ptx_ctx* ctx, float* replay_ms, float* accum_ms);

/* ---- the map objects of a replica: getRoot() (micromerge.ts:443-449) ----
 * applyOp on a map object (micromerge.ts:572-602) keeps, per key, the op with the largest opId (compareOpIds): last writer wins;
 * "del" removes the key, makeMap / makeList put a child object there.  ptx_root_map resolves, per replica log, every (object, key)
 * the log's PTX_ACT_MAPSET / PTX_ACT_MAPDEL / PTX_ACT_MAKELIST rows write: one ptx_root_entry per pair = the winning row.  An op
 * on an object that does not exist when it is applied (micromerge.ts:538-540 "Object does not exist"), or a key op on a list
 * object, fails the log with PTX_ERR_ELEM_NOT_FOUND (first failing row in first_bad_row).  Entries of log l are
 * entries[entry_off[l] .. entry_off[l] + logs[l].n_entries), in no particular order.  Owned by the library until ptx_root_maps_free. */
typedef struct ptx_root_entry {
    uint64_t obj;    /* the map: 0 = root, else the opId of its makeMap */
    uint32_t key;    /* key id */
    uint32_t row;    /* the winning row of the log (its op_id is the child's object id for PTX_MAPV_MAP / PTX_MAPV_LIST) */
    uint32_t kind;   /* PTX_MAPV_*: PTX_MAPV_DELETED = the key is absent */
    uint32_t value;  /* payload of the winning row (PTX_MAPV_SCALAR: value id) */
} ptx_root_entry;
typedef struct ptx_root_log {
    uint32_t status;        /* PTX_OK, PTX_ERR_ELEM_NOT_FOUND, PTX_ERR_CAPACITY (more map ops than the on-chip table holds) */
    uint32_t n_entries;
    uint32_t first_bad_row; /* 0xFFFFFFFF when status == PTX_OK */
    uint32_t reserved;
} ptx_root_log;
typedef struct ptx_root_maps {
    uint32_t n_logs;
    uint32_t reserved;
    const uint64_t* entry_off;     /* [n_logs + 1] */
    const ptx_root_log* logs;      /* [n_logs] */
    const ptx_root_entry* entries;
    void* owner;
} ptx_root_maps;
ptx_status ptx_root_map(ptx_ctx* ctx, const ptx_dbatch* b, ptx_root_maps* out);
void ptx_root_maps_free(ptx_root_maps* m);

/* ---- on-device change(): op logs generated in HBM ----
 * The workload of the reference's fuzzer (test/fuzz.ts:115-205) in its seeded form PTXGEN (oracle/ptxgen.js): per
 * document `replicas` replicas; every step a random replica makes one change() (micromerge.ts:308-441: insert /
 * delete / addMark / removeMark given by visible indexes, resolved to element ids incl. lookAfterTombstones :762-805
 * and changeMark peritext.ts:458-501), then two random replicas exchange what the other lacks with applyChange (:499),
 * retrying in the reference's order on the causal RangeError; a full sync ends the document.  Document `first_doc + i`
 * of seed `seed` is, change for change, the one oracle/ptxgen.js generates for (seed, first_doc + i).
 * String tables of a generated batch are fixed: insert payload = the character's code, link payload = letter index of
 * "<A-Z>.com", comment payload = rank of "comment-<k>" in string order among the document's n_comments ids,
 * actors "doc1".."doc<replicas>". */
typedef struct ptx_gen_config {
    uint32_t replicas;      /* 1..8 */
    uint32_t ops_per_log;   /* ops of every replica log (the makeList row comes on top) */
    uint32_t mix[4];        /* percent of insert, delete, addMark, removeMark steps */
    uint32_t n_mark_types;  /* 0..4 */
    uint8_t mark_types[4];  /* PTX_MARK_* the mark steps draw from, in the workload's order */
    uint32_t seed;
    uint32_t first_doc;
    uint32_t n_docs;
    uint32_t list_cap;      /* list elements (incl. tombstones) per replica the on-chip state holds; 0 = ops_per_log + 8 (always enough) */
    char initial_text[16];  /* NUL-terminated ASCII; "" = "ABCDE" (generateDocs.ts:11-42) */
} ptx_gen_config;
typedef struct ptx_gen_info {
    uint32_t n_docs;
    float kernel_ms;            /* duration of the generator launch (HIP events) */
    const uint32_t* n_comments; /* [n_docs] */
    void* owner;
} ptx_gen_info;
/* Generate n_docs documents (n_docs * replicas logs, document-major) as a resident batch, envelope and headers
 * included, ready for ptx_merge.  PTX_ERR_CAPACITY: some document outgrew list_cap (or the LDS). */
ptx_status ptx_generate(ptx_ctx* ctx, const ptx_gen_config* cfg, ptx_dbatch** out, ptx_gen_info* info);
void ptx_gen_info_free(ptx_gen_info* info);
/* ---- cursors: Micromerge.getCursor / resolveCursor (micromerge.ts:465-477) for many replicas ----
 * Query q names a replica log and is either
 *   PTX_CURSOR_RESOLVE  arg = the cursor's elemId (counter << 32 | actorRank)  ->  out = visible elements BEFORE that element
 *                       (findListElement(...).visible, :731-755; the element itself may be a tombstone — a cursor survives the
 *                       deletion of its character); PTX_ERR_ELEM_NOT_FOUND for an id that names no list element (:752)
 *   PTX_CURSOR_GET      arg = a visible index  ->  out = elemId of the index-th visible element (getListElementId, :762-805);
 *                       PTX_ERR_INDEX_OOB past the end (:804)
 * `r` = ptx_merge of `b` WITH elem_rank, complete.  All arrays are HOST memory, one entry per query; status_out[q] may also be
 * the log's merge status (a replica the reference threw on has no cursors) or PTX_ERR_CAPACITY.  The call synchronises. */
enum { PTX_CURSOR_RESOLVE = 0, PTX_CURSOR_GET = 1 };
ptx_status ptx_resolve_cursors(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, uint32_t n_queries, const uint32_t* q_log, const uint8_t* q_kind,
                               const uint64_t* q_arg, uint64_t* out, uint32_t* status_out);

/* ---- change(): caller-supplied InputOperations made into Changes on the device ----
 * Replaces `doc.change(ops: InputOperation[])` (micromerge.ts:308-441; InputOperation :133-148) for MANY replicas at once:
 * log l of `base` is a replica's op log as applied so far, the InputOperations of log l are resolved against THAT replica's
 * state (getListElementId incl. lookAfterTombstones :762-805, changeMark peritext.ts:458-501) into id-based ops and returned as
 * new Changes {actor, seq = clock + 1, deps = the clock before, startOp = maxOp + 1, ops} — one Change per entry of chg_off.
 * Columns (HOST pointers), one row per InputOperation:
 *   action      PTX_IN_INSERT {index, values}   PTX_IN_DELETE {index, count}   PTX_IN_ADDMARK / PTX_IN_REMOVEMARK {startIndex,
 *               endIndex, markType, attrs}      PTX_IN_MAKELIST {key: "text"} (only on a log without one)
 *   index       insert / delete: index            marks: startIndex
 *   count       insert: number of values          delete: count        marks: endIndex
 *   payload     insert: position of its first value in `values`        link: url id        comment: doc-local comment id
 *   mark_type   PTX_MARK_*
 * `actor[l]` = actorRank of the replica behind log l (ranks as in the op ids of `base`).  Ids follow the tables of `base`: a new
 * comment id must already have its rank (the caller encodes the document with the ids it is about to use). */
enum { PTX_IN_INSERT = 0, PTX_IN_DELETE = 1, PTX_IN_ADDMARK = 2, PTX_IN_REMOVEMARK = 3, PTX_IN_MAKELIST = 4,
       /* on a MAP object (micromerge.ts:400-425): {action: "set", key, value} / makeMap / makeList -> one PTX_ACT_MAPSET row, {action: "del",
        * key} -> one PTX_ACT_MAPDEL row.  index = the map object the host resolved the path to (getObjectIdForPath, :446-463): 0 = the
        * root map, PTX_IN_OBJ_NEW | k = the object made by row k of THIS log's output (a makeMap earlier in the same call), else counter
        * << 12 | actor rank of the makeMap that created it; count = key id, mark_type = PTX_MAPV_*, payload = value id */
       PTX_IN_MAPSET = 5, PTX_IN_MAPDEL = 6 };
#define PTX_IN_OBJ_NEW 0x80000000u
typedef struct ptx_input_ops {
    uint32_t n_logs;            /* == logs of the base batch */
    uint32_t max_actors;        /* actors of a document = row stride of the deps the new Changes carry (must equal the base
                                   batch's when that carries the envelope) */
    const uint64_t* chg_off;    /* [n_logs + 1] Changes to make per log (a log may make none) */
    const uint64_t* op_off;     /* [n_changes + 1] InputOperations per Change */
    const uint8_t* action;      /* [n_input_ops] PTX_IN_* */
    const uint8_t* mark_type;   /* [n_input_ops] */
    const uint32_t* index;      /* [n_input_ops] */
    const uint32_t* count;      /* [n_input_ops] */
    const uint32_t* payload;    /* [n_input_ops] */
    const uint32_t* values;     /* [n_values] value ids of the inserts */
    uint64_t n_values;
    const uint32_t* actor;      /* [n_logs] */
} ptx_input_ops;
/* `merged` = ptx_merge of `base` WITH elem_rank, complete (the call synchronises).  *made = a resident batch of n_logs logs
 * holding ONLY the new Changes (rows + envelope + headers), ready for ptx_batch_append_device / ptx_batch_download.
 * status_out[l] (caller memory, [n_logs]): PTX_OK, the log's merge status (a broken replica cannot make changes),
 * PTX_ERR_INDEX_OOB (the reference's RangeError, micromerge.ts:804), PTX_ERR_BAD_OP (no text list / a second makeList /
 * unknown action) or PTX_ERR_CAPACITY; a failed log makes NO change (the reference leaves the replica half-mutated: the ops
 * before the throw stay applied although no Change was returned — not reproduced). */
ptx_status ptx_change(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_dresult* merged, const ptx_input_ops* in, ptx_dbatch** made, uint32_t* status_out);
/* Streaming append with `more` already resident (e.g. the output of ptx_change): log l of *out = log l of `base` + log l of `more`. */
ptx_status ptx_batch_append_device(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_dbatch* more, ptx_dbatch** out);

/* ---- sync of replica logs: getMissingChanges + applyChanges (test/merge.ts:4-38; test/fuzz.ts:181-199 calls them in both directions after every
 * edit) for MANY (source, target) pairs at once, the logs staying resident ----
 * Pair p = (src_log[p], dst_log[p]) (HOST arrays), two replicas of the same document (they share the actor ranks).  Per pair, pinned to the reference:
 *   clocks        clock[a] = the largest seq of actor a in a log, 0 = absent (exact lo | hi << 16 with chg_env_hi)
 *   missing bag   the actors in the order of their FIRST APPEARANCE in the source log (the key order of source.clock, merge.ts:29); per actor the source's
 *                 changes with seq > the target's clock[a], in log order; an actor the target never saw contributes all of them (merge.ts:30-32)
 *   retry order   the queue of merge.ts:7-20: take the head, admit it as applyChange does (micromerge.ts:499-511: seq == clock[actor] + 1 and clock[b] >=
 *                 deps[b] for every non-zero dep, the own actor's included), push it to the back on failure
 *   the guard     merge.ts:18 throws once the 10 002nd attempt has been made, also when that attempt emptied the queue: a pair that takes more than
 *                 max_attempts attempts (10 001 = the reference; 0 = unbounded) is PTX_ERR_SYNC_NOT_CONVERGED, and so is — whatever max_attempts — a pass
 *                 that admits nothing (a source log no replica could have applied: the reference spins into its guard, this call terminates)
 * *more = a resident batch of base's n_logs logs, envelope (the wide column iff `base` has one), max_actors and computed headers: log dst_log[p] holds the
 * admitted changes of pair p IN ADMITTED ORDER with their op rows, every other log is empty — made for ptx_batch_append_device(base, more).  All pairs read
 * `base` as it is: a bidirectional sync is the two pairs (l, r) and (r, l) of one call (what r received from l is never missing for l: fuzz.ts:198-199).  A log
 * may be a source any number of times and a source and a target at once; a log that is a target twice is PTX_ERR_INVALID_ARG; src == dst is an empty log.
 * status_out[p] (caller memory): PTX_OK, PTX_ERR_SYNC_NOT_CONVERGED, PTX_ERR_CAPACITY (a narrow envelope with a saturated value, 65 535, in either log) or
 * PTX_ERR_BAD_OP (an actor rank >= max_actors); a failed pair contributes an EMPTY log and `base` is never touched (the reference leaves the target
 * half-updated — not reproduced).  merge.ts:15 catches every error, op-level ones too; this call looks at the ENVELOPE only: a change whose ops would throw is
 * ordered like any other and the grown log reports its op-level status at its merge.  A batch without the envelope is PTX_ERR_INVALID_ARG.  No bound on the
 * logs below the batch format's own; the per-actor tables (24 bytes per actor) must fit one CU's LDS.  The call synchronises. */
ptx_status ptx_sync_replicas(ptx_ctx* ctx, const ptx_dbatch* base, uint32_t n_pairs, const uint32_t* src_log, const uint32_t* dst_log, uint32_t max_attempts,
                             ptx_dbatch** more, uint32_t* status_out);

/* ---- documents at a past version: resident logs cut at vector clocks or at a prefix of their own history, the logs staying resident ----
 * Cut c reads the source log src_log[c] (HOST array) of `base`, a batch with the Change envelope; the actor ranks are the batch's own.  Per call either
 *   clock cuts    clocks[c * max_actors + a] (HOST, u32): a change of actor a is KEPT iff seq <= clocks[c][a] — micromerge.ts:511 sets clock[actor] = seq at every
 *                 admission, so that is the set a replica with this clock holds.  0 keeps none of the actor, PTX_VERSION_ALL all; exact lo | hi << 16 where the
 *                 batch has chg_env_hi.  A clock no replica could have had — a kept change with a non-zero deps[b], b not its own actor, > clocks[c][b] — is that
 *                 cut's PTX_ERR_MISSING_DEP: applyChange throws "Missing dependency" (micromerge.ts:505-508) at that change on a fresh Micromerge.  Checked on the
 *                 envelope alone; the source log is not re-admitted (an inadmissible source shows at the cut log's merge, as a grown log does after a sync), or
 *   prefix cuts   prefix[c] = k (HOST) keeps the first min(k, n) changes: the version the replica itself was at after its k-th applyChange / change().
 * Both or neither given is PTX_ERR_INVALID_ARG, as are src_log[c] >= n_logs and a batch without the envelope.
 * *out = a resident batch of n_cuts logs, base's max_actors, the wide column iff `base` has one, computed headers and launch shape: log c = the kept changes of
 * cut c IN LOG ORDER with their op rows, chg_hdr and envelope rows (admissible in that order for a closed clock: every dep of a kept change stands before it
 * and is kept).  With PTX_VERSIONS_THEN_REST the dropped changes follow the kept ones, also in log order — a stable partition that merges to the source's
 * present document — and first_row_out[c] is what ptx_replay_patches_from takes as first_row: the stream it returns is the Patch[] from version V to the present.
 * Per cut (caller memory, [n_cuts]; each may be NULL except status_out): status_out PTX_OK, PTX_ERR_MISSING_DEP, PTX_ERR_CAPACITY (a narrow envelope with a
 * saturated value, 65 535, in the source log) or PTX_ERR_BAD_OP (an actor rank >= max_actors); n_kept_out the changes kept; first_row_out their op rows;
 * clocks_out[c * max_actors + a] the largest kept seq of actor a, 0 = none (how a caller of a prefix cut learns the version's clock).  A failed cut
 * contributes an EMPTY log and zero outputs; `base` is never touched.  A log may be the source of any number of cuts; n_cuts == 0 is an empty batch.  The call
 * synchronises. */
#define PTX_VERSION_ALL 0xFFFFFFFFu
#define PTX_VERSIONS_THEN_REST 1u
ptx_status ptx_batch_at_versions(ptx_ctx* ctx, const ptx_dbatch* base, uint32_t n_cuts, const uint32_t* src_log, const uint32_t* clocks, const uint32_t* prefix,
                                 uint32_t flags, ptx_dbatch** out, uint32_t* status_out, uint32_t* n_kept_out, uint32_t* first_row_out, uint32_t* clocks_out);

/* ---- document text: what getTextWithFormatting returns is {text, marks}[] (peritext.ts:337-395; addCharactersToSpans :438-455) ----
 * ptx_result carries value IDS, and a span's `start` is an ELEMENT index: a value is any JS string (one character, a pasted paragraph inserted as one value —
 * test/micromerge.ts:202 —, the empty string, half of a surrogate pair), so a host had to join the text one table lookup per visible element.  With the string
 * table resident the device assembles ONE UTF-16 buffer per downloaded range, and a host builds each FormatSpanWithText.text with a single slice:
 *   text of log l     text[text_off[l] .. text_off[l + 1]) = the concatenation of string[values[i]] over the log's n_visible elements in document order
 *   text of span k    the log's text from span_unit[span_off[l] + k] to span_unit[span_off[l] + k + 1] (the last span: to the log's length text_off[l + 1] -
 *                     text_off[l]).  An element whose string is empty is still an element: a span made only of such elements has span_unit equal to its successor's.
 * Units are UTF-16 CODE UNITS (JS string semantics, not code points); lone surrogates are legal and copied as they are.
 * Per-log status (the other logs of the range are never affected):
 *   the log's merge status   a log the merge failed has no text and no spans
 *   PTX_ERR_BAD_OP           a value id >= n_strings.  Every id is checked before anything is read through it: never an out-of-range read.  No text; the spans of
 *                            the merge stay counted in span_off (it equals ptx_result.span_off of the same range), their span_unit is 0
 *   PTX_ERR_CAPACITY         the log's text reaches 2^32 code units (span_unit is 32 bits wide).  No text, as above
 * n_logs == 0 returns an empty result (text_off = span_off = {0}); a range outside the batch is PTX_ERR_INVALID_ARG.  `r` = ptx_merge of `b`, enqueued on this
 * context's stream or complete; elem_rank is not needed (PTX_FLAG_NO_ELEM_RANK contexts work).  The insert payloads of a batch made by ptx_generate are character
 * codes: a table of 128 one-unit strings (or 65 536 of them) serves it. */
typedef struct ptx_dstrings ptx_dstrings;   /* a string table resident in HBM */
/* units: the UTF-16 code units of all strings back to back; off: [n_strings + 1], off[0] == 0, monotonic (else PTX_ERR_INVALID_ARG).  HOST pointers; copied before
 * the call returns.  n_strings == 0 is legal (every value id is then PTX_ERR_BAD_OP). */
ptx_status ptx_strings_upload(ptx_ctx* ctx, const uint16_t* units, const uint64_t* off, uint32_t n_strings, ptx_dstrings** out);
void ptx_strings_free(ptx_ctx* ctx, ptx_dstrings* s);
typedef struct ptx_text {
    uint32_t n_logs;
    uint32_t reserved;
    float kernel_ms;               /* HIP-event duration of the length (+ offset scan) and assemble launches */
    uint32_t reserved2;
    const uint32_t* status;        /* [n_logs] PTX_OK, the log's merge status, PTX_ERR_BAD_OP, PTX_ERR_CAPACITY */
    const uint64_t* text_off;      /* [n_logs + 1] code units */
    const uint16_t* text;          /* [text_off[n_logs]] */
    const uint64_t* span_off;      /* [n_logs + 1] == ptx_result.span_off of the same range */
    const uint32_t* span_unit;     /* [span_off[n_logs]] code-unit offset, within the log's text, of the first element of span k */
    void* owner;
} ptx_text;
/* The text of the logs [first_log, first_log + n_logs).  Synchronises.  Owned by the library until ptx_text_free. */
ptx_status ptx_result_text_range(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs, ptx_text* out);
void ptx_text_free(ptx_text* t);

/* ---- find in the documents' text without downloading it ----
 * The reference has no search: its documents are JS strings (getTextWithFormatting, peritext.ts:337-395) and a caller writes text.indexOf(pattern, from).  This
 * is String.prototype.indexOf applied repeatedly from p + 1, over the text ptx_result_text_range would return for the same range, which stays on the device:
 *   match              a position p with 0 <= p <= L - m and text[p + i] == pattern[i] for all i < m (L: the log's text length in code units, m = n_pattern)
 *   overlapping        ALL such positions are reported, overlapping ones included: "aaaa" holds "aa" three times
 *   code units         the comparison is over UTF-16 code units, not code points: a pattern that is a lone high surrogate matches the first half of a pair, a
 *                      pair split over two elements matches a two-unit pattern
 *   PTX_FIND_ASCII_NOCASE   'A'..'Z' compare equal to 'a'..'z', in text and pattern; no other unit is folded (U+0130, U+212A match neither i nor k)
 *   order and the cap  hit_unit ascends within a log; the listed hits are the FIRST max_hits_per_log of them; n_matches always counts all of them
 *   count only         max_hits_per_log == 0: empty hit arrays — "which documents mention it"
 *   log boundaries     a match never reaches from one log's text into the next log's
 *   element mapping    element e holds unit u iff pre[e] <= u < pre[e + 1], pre = the exclusive scan of the elements' string lengths.  hit_start = the visible
 *                      index of the element that holds the match's first unit, hit_end = that of its last unit + 1 — exclusive, as changeMark's endIndex
 *                      (peritext.ts:491-497): delete {index: hit_start, count: hit_end - hit_start} and addMark {startIndex: hit_start, endIndex: hit_end} take
 *                      them as they are, ptx_resolve_cursors (PTX_CURSOR_GET) turns them into elemIds.  An element whose string is empty holds no unit: it is
 *                      never a hit_start, but may lie inside [hit_start, hit_end).  A match inside one multi-unit element (a pasted paragraph inserted as one
 *                      value) has hit_end == hit_start + 1; hit_unit tells where it sits
 *   per-log status     exactly ptx_text.status of the same range, under the same guarantee (every value id is checked before anything is read through it): the
 *                      log's merge status, PTX_ERR_BAD_OP for a value id >= n_strings, PTX_ERR_CAPACITY.  A log that is not PTX_OK has zero matches; the other
 *                      logs are untouched
 * PTX_ERR_INVALID_ARG: n_pattern == 0, n_pattern > PTX_FIND_PATTERN_MAX, an unknown flag bit, a range outside the batch.  n_logs == 0 returns an empty result
 * (hit_off = {0}).  `pattern` is a HOST pointer, copied before the call returns.  elem_rank is not needed (PTX_FLAG_NO_ELEM_RANK contexts work).  Synchronises. */
#define PTX_FIND_PATTERN_MAX 256u      /* code units */
#define PTX_FIND_ASCII_NOCASE 1u
typedef struct ptx_matches {
    uint32_t n_logs;
    uint32_t n_pattern;
    float kernel_ms;               /* HIP events around every launch of the call */
    uint32_t reserved;
    const uint32_t* status;        /* [n_logs] exactly ptx_text.status of the same range */
    const uint32_t* n_matches;     /* [n_logs] ALL matches of the log, listed or not */
    const uint64_t* hit_off;       /* [n_logs + 1] listed hits: min(n_matches[l], max_hits_per_log) per log */
    const uint32_t* hit_unit;      /* [hit_off[n_logs]] code-unit offset of the match within the log's text, ascending per log */
    const uint32_t* hit_start;     /* ... visible index of the element that holds the match's first unit */
    const uint32_t* hit_end;       /* ... visible index of the element that holds its last unit, + 1 */
    void* owner;
} ptx_matches;
/* Owned by the library until ptx_matches_free. */
ptx_status ptx_result_find_text(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs,
                                const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log, ptx_matches* out);
void ptx_matches_free(ptx_matches* m);

/* ---- the text of element ranges, with their formatting, without downloading the documents ----
 * The reference's caller slices what getTextWithFormatting returned; a hit of ptx_result_find_text, a comment interval (ptx_cinterval) and a span are ranges of
 * visible ELEMENT indexes of a log.  This returns the text and the span rows of many such ranges of many logs in one call; the documents' text stays on the
 * device.  Log l of the range has the slices slice_off[l] .. slice_off[l + 1] of slice_start / slice_end.
 *   clamping           Array.prototype.slice(start, end) over the log's n_visible elements, for non-negative arguments: elem_end = min(end, n_visible),
 *                      elem_start = min(start, n_visible); elem_start >= elem_end after that is the EMPTY slice, reported as elem_start == elem_end ==
 *                      min(start, n_visible).  0xFFFFFFFF is a legal bound: a context window [hit_start - c, hit_end + c) needs no clamping by the caller
 *                      beyond saturating the subtraction at 0
 *   order              the slices of a log may come in any order, overlap, nest and repeat; every output follows the caller's order
 *   text               slice k's code units are text[unit_off[k] .. unit_off[k + 1]) = the concatenation of string[values[i]] for i in [elem_start, elem_end).
 *                      UTF-16 code units, as ptx_text: a slice that cuts a surrogate pair split over two elements returns a lone surrogate; an element whose
 *                      string is empty contributes nothing but is still an element
 *   span rows          slice k's rows are sspans / sspan_unit [sspan_off[k] .. sspan_off[k + 1]).  For a non-empty slice [a, b) they are the log's span rows with
 *                      start < b whose successor's start (the last row's: n_visible) is > a, in order, `attr` unchanged; the first row's start is raised to a.
 *                      `start` stays a DOCUMENT element index — the log's cintervals, addMark {startIndex} and cursor requests take it as it is;
 *                      sspan_unit is the code-unit offset of that start within the SLICE's text.  A row ends where the next one starts, the last at elem_end.
 *                      A slice made only of empty-string elements has zero units and still its rows.  An empty slice has zero rows.  Comment ids are not
 *                      repeated: a row with PTX_ATTR_COMMENT is resolved against the log's cintervals, as for the full result
 *   per-log status     exactly ptx_text.status of the same range, under the same guarantee (every value id is checked before anything is read through it).  A
 *                      log that is not PTX_OK has empty slices without rows, elem_start == elem_end == 0; the other logs are untouched
 * PTX_ERR_INVALID_ARG: a range outside the batch; slice_off[0] != 0 or a slice_off that decreases; slice_off == NULL with n_logs > 0; a NULL slice_start or
 * slice_end with slices present; more than 0xFFFFFFFF slices.  n_logs == 0 or zero slices returns an empty result (unit_off = sspan_off = {0}).  The three
 * slice arrays are HOST pointers, copied before the call returns.  elem_rank is not needed (PTX_FLAG_NO_ELEM_RANK contexts work).  Synchronises. */
typedef struct ptx_slices {
    uint32_t n_logs;
    uint32_t n_slices;
    float kernel_ms;               /* HIP events around every launch of the call, the text passes included */
    uint32_t reserved;
    const uint32_t* status;        /* [n_logs] exactly ptx_text.status of the same range */
    const uint32_t* elem_start;    /* [n_slices] the range after clamping */
    const uint32_t* elem_end;      /* ... */
    const uint64_t* unit_off;      /* [n_slices + 1] code units */
    const uint16_t* text;          /* [unit_off[n_slices]] the slices' text back to back, in the caller's order */
    const uint64_t* sspan_off;     /* [n_slices + 1] rows of the two arrays below */
    const ptx_span* sspans;        /* [sspan_off[n_slices]] start: a document element index, >= elem_start of its slice; attr: the log's row's */
    const uint32_t* sspan_unit;    /* ... code-unit offset of `start` within the slice's text */
    void* owner;
} ptx_slices;
/* Owned by the library until ptx_slices_free. */
ptx_status ptx_result_text_slices(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs,
                                  const uint64_t* slice_off, const uint32_t* slice_start, const uint32_t* slice_end, ptx_slices* out);
void ptx_slices_free(ptx_slices* m);

/* ---- a resident text view: search and snippets without re-assembling the text ----
 * ptx_result_find_text and ptx_result_text_slices assemble the documents' text per call, and a slice call rebuilds the element prefix as well.  A view holds
 * both for the logs [first_log, first_log + n_logs) of ONE merge; it is made once and queried any number of times.  It owns, in device memory of its own (not the
 * context's pool of small blocks), what ptx_result_text_range returns for the range — status, text_off, span_off, text, span_unit — and, for every log that is
 * PTX_OK, the exclusive element prefix pre[0 .. n_visible] (pre[e] = the code-unit offset of visible element e in the log's text) with its offsets, and the
 * batch's row offsets of the range.
 *   cost               2 bytes per code unit + 4 per span row + 4 per visible element (+ 4 per good log) + 52 per log.  The 49 152 `rich4k` logs of DESIGN §3k:
 *                      184 MB of text + 367 MB of prefix
 *   lifetimes          once ptx_text_view_create has returned the view reads nothing of `b` or `s`: `s` may be freed.  It reads the span rows of `r` — and
 *                      nothing else of it: a log's n_visible is taken from the view's own prefix — in slice and snippet calls: `r` must outlive the view
 *                      and stay the merge it was made from (a ptx_merge into `r` after an append makes the view stale: free it and make a new one).  The
 *                      queries by format below (ptx_view_mark_runs, ptx_view_mark_snippets, ptx_view_find_in_marks) read the span rows too, and for
 *                      PTX_MARK_COMMENT additionally the result's per-log n_cintervals and its cintervals rows
 *   ptx_view_find_text / ptx_view_text_slices   every field of ptx_matches / ptx_slices equals what ptx_result_find_text / ptx_result_text_slices return for the
 *                      same (b, r, s, range) — kernel_ms excepted —, the argument errors are the same, plus PTX_ERR_INVALID_ARG for a NULL view.  No text pass
 *                      and no prefix pass runs
 *   ptx_view_find_snippets   find, then ONE snippet per listed hit, in hit order, without the hits leaving the device in between: n_slices == hit_off[n_logs],
 *                      slice k belongs to hit k.  The snippet of hit k is the slice [hit_start[k] - before, hit_end[k] + after) — the subtraction saturates at
 *                      0, the addition at 0xFFFFFFFF; `before` and `after` may be 0 or 0xFFFFFFFF — clamped exactly as ptx_result_text_slices clamps.
 *                      match_unit[k] = hit_unit[k] - pre[elem_start[k]] is the code-unit offset of the match within snippet k's text:
 *                      text[unit_off[k] + match_unit[k] .. + n_pattern) is the pattern (after folding under PTX_FIND_ASCII_NOCASE).  It cannot be derived
 *                      from element counts: an element may hold many units.  Overlapping hits give overlapping snippets, nothing is merged.
 *                      max_hits_per_log == 0 is the count-only answer with zero snippets
 * A range outside the batch is PTX_ERR_INVALID_ARG.  n_logs == 0 makes a legal empty view; every query on it returns the empty result of its ptx_result_* twin.
 * elem_rank is not needed (PTX_FLAG_NO_ELEM_RANK contexts work).  ptx_text_view_create and every query synchronise. */
typedef struct ptx_dview ptx_dview;
typedef struct ptx_view_desc {
    uint32_t n_logs;
    uint32_t first_log;
    uint64_t n_units;              /* code units of the range: text_off[n_logs] */
    uint64_t n_prefix_words;       /* words of the element prefix: the sum of n_visible + 1 over the logs that are PTX_OK */
    uint64_t bytes;                /* device memory the view holds */
    float kernel_ms;               /* HIP events around every launch of ptx_text_view_create */
    uint32_t reserved;
} ptx_view_desc;
typedef struct ptx_snippets {
    uint32_t n_logs;
    uint32_t n_pattern;
    float kernel_ms;               /* HIP events around every launch of the call */
    uint32_t n_slices;             /* == hit_off[n_logs] */
    const uint32_t* status;        /* [n_logs] as ptx_matches */
    const uint32_t* n_matches;     /* [n_logs] */
    const uint64_t* hit_off;       /* [n_logs + 1] */
    const uint32_t* hit_unit;      /* [n_slices] */
    const uint32_t* hit_start;
    const uint32_t* hit_end;
    const uint32_t* elem_start;    /* [n_slices] as ptx_slices, of the slice [hit_start - before, hit_end + after) */
    const uint32_t* elem_end;
    const uint64_t* unit_off;      /* [n_slices + 1] */
    const uint16_t* text;          /* [unit_off[n_slices]] */
    const uint64_t* sspan_off;     /* [n_slices + 1] */
    const ptx_span* sspans;        /* [sspan_off[n_slices]] */
    const uint32_t* sspan_unit;
    const uint32_t* match_unit;    /* [n_slices] code-unit offset of the match within the snippet's text */
    void* owner;
} ptx_snippets;
ptx_status ptx_text_view_create(ptx_ctx* ctx, const ptx_dbatch* b, const ptx_dresult* r, const ptx_dstrings* s, uint32_t first_log, uint32_t n_logs, ptx_dview** out);
void ptx_text_view_free(ptx_ctx* ctx, ptx_dview* v);
ptx_status ptx_view_info(ptx_ctx* ctx, const ptx_dview* v, ptx_view_desc* out);
/* Owned by the library until ptx_matches_free / ptx_slices_free / ptx_snippets_free. */
ptx_status ptx_view_find_text(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log, ptx_matches* out);
ptx_status ptx_view_text_slices(ptx_ctx* ctx, const ptx_dview* v, const uint64_t* slice_off, const uint32_t* slice_start, const uint32_t* slice_end, ptx_slices* out);
ptx_status ptx_view_find_snippets(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t max_hits_per_log,
                                  uint32_t before, uint32_t after, ptx_snippets* out);
void ptx_snippets_free(ptx_snippets* m);

/* ---- a resident text view queried by FORMAT: the runs of a mark, their text, a find inside them ----
 * "List every comment with the text it is anchored to", "every link and its text", "where is the bold text", "find this word, but only inside links".  The span
 * rows and comment intervals of the merge are on the device; the runs are chosen there and never come down before the slice passes or the hit filter read them.
 * A selector is (mark_type, id), mark_type one of PTX_MARK_*:
 *   PTX_MARK_STRONG / PTX_MARK_EM   id must be PTX_MARK_ANY_ID.  A span row matches iff its attr has the flag.  A run is a MAXIMAL sequence of consecutive matching
 *                      span rows of the log — two adjacent rows may both be strong and differ only in em —: [start of its first row, start of the row behind its
 *                      last row), the log's n_visible behind the last row (taken from the view's own prefix).  run_id is 0
 *   PTX_MARK_LINK      a row matches iff PTX_ATTR_LINK is set and (id == PTX_MARK_ANY_ID or (attr & PTX_ATTR_ID_MASK) == id).  A run also ends where the url id
 *                      changes: two adjacent links to different urls are two runs.  run_id is the url id.  An id > PTX_ATTR_ID_MASK that is not
 *                      PTX_MARK_ANY_ID is PTX_ERR_INVALID_ARG
 *   PTX_MARK_COMMENT   the runs are the log's cintervals rows whose id equals `id`, with PTX_MARK_ANY_ID all of them, in the RESULT'S OWN ORDER (id, start) — which
 *                      is NOT ascending start across ids: the intervals of one id ascend, those of the next id start over.  run_id is the doc-local comment id.
 *                      A span with PTX_ATTR_COMMENT and no covering interval (`comment: []`) belongs to no run
 *   order and cap      the runs of strong, em and link ascend by start within a log.  The listed runs are the FIRST max_runs_per_log of the log; n_runs counts
 *                      ALL of them; max_runs_per_log == 0 is the count-only answer
 *   units              run_unit = pre[run_start], run_len = pre[run_end] - pre[run_start] (pre: the view's element prefix).  A run made only of empty-string
 *                      elements has run_len == 0 and is still a run
 *   per-log status     exactly ptx_matches.status of the view.  Only a log that is PTX_OK has runs
 *   ptx_view_mark_snippets   ONE slice per listed run, in run order, without the runs leaving the device in between: n_slices == run_off[n_logs].  The slice of run
 *                      k is [run_start[k] - before, run_end[k] + after), saturating and clamped exactly as ptx_view_find_snippets windows a hit; the slice
 *                      fields are those of ptx_snippets.  match_unit[k] = pre[run_start[k]] - pre[elem_start[k]]: where the run begins inside the snippet's
 *                      text.  With before == after == 0 the snippet IS the run's text — the text each comment is anchored to
 *   ptx_view_find_in_marks   the hits of ptx_view_find_text with max_hits_per_log = 0xFFFFFFFF whose [hit_start, hit_end) lies inside ONE run of the selector:
 *                      run_start <= hit_start && hit_end <= run_end.  Containment is over ELEMENTS, because marks are per element: it is the range addMark
 *                      {startIndex: hit_start, endIndex: hit_end} would take.  n_matches counts the contained hits, the listed ones are the first
 *                      max_hits_per_log of them; order and every other field as ptx_view_find_text.  PTX_MARK_COMMENT needs a specific id: PTX_MARK_ANY_ID
 *                      there is PTX_ERR_INVALID_ARG, because a log's intervals of different ids are not sorted by start.  More than 2^32 - 1 matches in the view
 *                      is PTX_ERR_CAPACITY, as for find
 *   lifetimes          as for the view's other queries: `r` must outlive the view and stay the merge it was made from.  These calls read its span rows; comment
 *                      queries additionally read its per-log n_cintervals and its cintervals rows
 * PTX_ERR_INVALID_ARG: a NULL view, an unknown mark_type, the id errors above, and for ptx_view_find_in_marks the argument errors of ptx_view_find_text.  An empty
 * view returns the empty result (run_off = {0}).  elem_rank is not needed (PTX_FLAG_NO_ELEM_RANK contexts work).  Every call synchronises. */
#define PTX_MARK_ANY_ID 0xFFFFFFFFu
typedef struct ptx_mark_runs {
    uint32_t n_logs;
    uint32_t mark_type;
    float kernel_ms;               /* HIP events around every launch of the call */
    uint32_t reserved;
    const uint32_t* status;        /* [n_logs] as ptx_matches */
    const uint32_t* n_runs;        /* [n_logs] ALL runs of the log, listed or not */
    const uint64_t* run_off;       /* [n_logs + 1] listed runs: min(n_runs[l], max_runs_per_log) per log */
    const uint32_t* run_start;     /* [run_off[n_logs]] visible index of the run's first element */
    const uint32_t* run_end;       /* ... of its last element, + 1 */
    const uint32_t* run_id;        /* ... 0 (strong, em), the url id (link), the doc-local comment id (comment) */
    const uint32_t* run_unit;      /* ... code-unit offset of the run within the log's text */
    const uint32_t* run_len;       /* ... its length in code units */
    void* owner;
} ptx_mark_runs;
typedef struct ptx_mark_snippets {
    uint32_t n_logs;
    uint32_t mark_type;
    float kernel_ms;
    uint32_t n_slices;             /* == run_off[n_logs] */
    const uint32_t* status;
    const uint32_t* n_runs;
    const uint64_t* run_off;
    const uint32_t* run_start;
    const uint32_t* run_end;
    const uint32_t* run_id;
    const uint32_t* run_unit;
    const uint32_t* run_len;
    const uint32_t* elem_start;    /* [n_slices] as ptx_snippets, of the slice [run_start - before, run_end + after) */
    const uint32_t* elem_end;
    const uint64_t* unit_off;      /* [n_slices + 1] */
    const uint16_t* text;          /* [unit_off[n_slices]] */
    const uint64_t* sspan_off;     /* [n_slices + 1] */
    const ptx_span* sspans;        /* [sspan_off[n_slices]] */
    const uint32_t* sspan_unit;
    const uint32_t* match_unit;    /* [n_slices] code-unit offset of the run's first unit within the snippet's text */
    void* owner;
} ptx_mark_snippets;
/* Owned by the library until ptx_mark_runs_free / ptx_mark_snippets_free / ptx_matches_free. */
ptx_status ptx_view_mark_runs(ptx_ctx* ctx, const ptx_dview* v, uint32_t mark_type, uint32_t id, uint32_t max_runs_per_log, ptx_mark_runs* out);
void ptx_mark_runs_free(ptx_mark_runs* m);
ptx_status ptx_view_mark_snippets(ptx_ctx* ctx, const ptx_dview* v, uint32_t mark_type, uint32_t id, uint32_t max_runs_per_log, uint32_t before, uint32_t after,
                                  ptx_mark_snippets* out);
void ptx_mark_snippets_free(ptx_mark_snippets* m);
ptx_status ptx_view_find_in_marks(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, uint32_t mark_type, uint32_t id,
                                  uint32_t max_hits_per_log, ptx_matches* out);

/* ---- find and replace on a resident text view: hits into change() input ----
 * The reference's editor turns a ProseMirror ReplaceStep into a `delete` followed by an `insert` at the same index (bridge.ts:425-446).  This answers, for every
 * log of a view: which matches String.prototype.replaceAll(pattern, ...) would replace, and the InputOperations that do it — the `in` of ptx_change.
 *   matches            exactly those of ptx_view_find_text with max_hits_per_log = 0xFFFFFFFF, flags included (PTX_FIND_ASCII_NOCASE), over the same text
 *   chosen matches     greedy, leftmost, non-overlapping, over ALL matches of the log: the first match is chosen, and after a chosen match at unit u the next
 *                      chosen one is the first with hit_unit >= u + n_pattern — what replaceAll and Python's str.replace do.  The choice does not look at
 *                      element boundaries
 *   replaceable        a chosen match is replaceable iff it covers whole elements: pre[hit_start] == hit_unit and pre[hit_end] == hit_unit + n_pattern (the view
 *                      holds pre[0 .. n_visible]).  A chosen match that starts or ends inside a multi-unit element is skipped and counted (n_chosen -
 *                      n_replaced); it still blocks the matches it overlaps.  Empty-string elements inside [hit_start, hit_end) go with the match; those
 *                      directly before or after it stay
 *   ops                a log with R > 0 replaceable matches gets ONE Change.  Its matches are taken in DESCENDING hit order, so no index needs adjusting; each
 *                      gives PTX_IN_DELETE {index: hit_start, count: hit_end - hit_start} and then, if n_replacement > 0, PTX_IN_INSERT {index: hit_start,
 *                      count: n_replacement, payload: 0} — the order of bridge.ts:425-446.  `values` is the caller's n_replacement value ids once, shared by
 *                      every insert: one element per id.  The replacement is never rescanned
 *   shape              ptx_change demands in->n_logs == base->n_logs, so the call takes n_batch_logs: ops.n_logs == n_batch_logs, chg_off has n_batch_logs + 1
 *                      entries, view log l is batch log first_log + l, and logs outside the view's range make no Change.  ops.actor and ops.max_actors are
 *                      left NULL / 0 for the caller to fill in
 *   per-log status     the view's (ptx_matches.status), and PTX_ERR_CAPACITY where the Change would make more than the PTX_CHANGE_ROWS_MAX rows ptx_change accepts
 *                      per log: rows = the sum of hit_end - hit_start + R * n_replacement.  A log that is not PTX_OK gets no ops; the counts of a
 *                      PTX_ERR_CAPACITY log are still reported
 * PTX_ERR_INVALID_ARG: the argument errors of ptx_view_find_text; n_replacement > PTX_CHANGE_ROWS_MAX; n_replacement > 0 with a NULL `replacement`;
 * n_batch_logs < first_log + n_logs of the view.  More than 2^32 - 1 matches in the view is PTX_ERR_CAPACITY, as for find.  An empty view returns an all-zero
 * plan (chg_off all 0, op_off = {0}).  `pattern` and `replacement` are HOST pointers, copied before the call returns.  elem_rank is not needed
 * (PTX_FLAG_NO_ELEM_RANK contexts work: the plan reads no elem_rank — ptx_change does).  Synchronises. */
#define PTX_CHANGE_ROWS_MAX 65534u     /* rows the Changes of ONE log may make in one ptx_change call */
typedef struct ptx_replace_plan {
    uint32_t n_logs;               /* of the view */
    uint32_t n_pattern;
    float kernel_ms;               /* HIP events around every launch of the call */
    uint32_t n_replacement;
    const uint32_t* status;        /* [n_logs] */
    const uint32_t* n_matches;     /* [n_logs] ALL matches of the log */
    const uint32_t* n_chosen;      /* [n_logs] the greedy, non-overlapping ones */
    const uint32_t* n_replaced;    /* [n_logs] those of them that cover whole elements */
    ptx_input_ops ops;             /* its pointers point into the plan's blocks */
    void* owner;
} ptx_replace_plan;
/* Owned by the library until ptx_replace_plan_free. */
ptx_status ptx_view_replace_plan(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, const uint32_t* replacement,
                                 uint32_t n_replacement, uint32_t n_batch_logs, ptx_replace_plan* out);
void ptx_replace_plan_free(ptx_replace_plan* m);

/* ---- InputOperations as a resident object: change() without the host in between ----
 * ptx_change takes its InputOperations from host memory: it walks every op and every offset there, downloads the headers of the base batch to size its launch
 * and uploads the ops.  A ptx_dinput_ops holds the same eleven arrays in device memory, and ptx_change_device does the walks there.
 *   ptx_input_ops_upload       copies the arrays of `host` (one copy out of pinned memory where they are small).  It reads chg_off[n_logs] and
 *                              op_off[n_changes] to learn the sizes and validates nothing else; chg_off / op_off / actor (n_logs > 0) and the five op columns
 *                              (n_input_ops > 0) must not be NULL.  Synchronises: the caller's arrays are free to go
 *   ptx_input_ops_wrap_device  adopts DEVICE columns the caller owns (torch tensors, say) and copies nothing: they must outlive the object and every call that
 *                              takes it.  The library cannot read the sizes, so they are arguments; n_values is the struct's field.  chg_off must hold
 *                              n_logs + 1 entries, op_off n_changes + 1, the op columns n_input_ops
 *   ptx_input_ops_download     a host copy, library-owned until ptx_host_input_ops_free
 *   ptx_change_device          ptx_change on the same arrays: the same call status, the same status_out, a `made` batch equal column for column, envelope and
 *                              headers included.  The argument errors ptx_change finds by walking the arrays — chg_off / op_off not starting at 0 or
 *                              decreasing, an insert pointing outside `values`, more than PTX_CHANGE_ROWS_MAX rows for one log — are found on the device and
 *                              fail the whole call with PTX_ERR_INVALID_ARG at its first wait, before any output is allocated: *made = NULL, status_out
 *                              untouched, ptx_last_error names the lowest offending entry or log.  One check more than ptx_change's, because the sizes of a
 *                              wrapped object are the caller's word: chg_off and op_off must END at n_changes and n_input_ops (PTX_ERR_INVALID_ARG; nothing is
 *                              read behind the columns in either case).  Three waits; between them nothing proportional to the ops or to the base batch's logs
 *                              crosses PCIe except status_out
 *   ptx_view_replace_plan_device  ptx_view_replace_plan with the ops left where the passes wrote them: status and the three count arrays come down in
 *                              `counts` (the pointers of counts->ops stay NULL; its n_logs, n_values and max_actors are filled), the op columns, chg_off,
 *                              op_off and the replacement's value ids stay on the device in *ops, with `actor` (HOST, [n_batch_logs], copied) and max_actors.
 *                              The argument errors of ptx_view_replace_plan, and a NULL `actor` with n_batch_logs > 0.  Free `counts` with
 *                              ptx_replace_plan_free and *ops with ptx_input_ops_free */
typedef struct ptx_dinput_ops ptx_dinput_ops;
typedef struct ptx_host_input_ops {
    ptx_input_ops ops;             /* HOST pointers into a library-owned block */
    uint64_t n_changes;
    uint64_t n_input_ops;
    void* owner;
} ptx_host_input_ops;
ptx_status ptx_input_ops_upload(ptx_ctx* ctx, const ptx_input_ops* host, ptx_dinput_ops** out);
ptx_status ptx_input_ops_wrap_device(ptx_ctx* ctx, const ptx_input_ops* device_columns, uint64_t n_changes, uint64_t n_input_ops, ptx_dinput_ops** out);
ptx_status ptx_input_ops_download(ptx_ctx* ctx, const ptx_dinput_ops* d, ptx_host_input_ops* out);
void ptx_host_input_ops_free(ptx_host_input_ops* h);
void ptx_input_ops_free(ptx_ctx* ctx, ptx_dinput_ops* d);
ptx_status ptx_change_device(ptx_ctx* ctx, const ptx_dbatch* base, const ptx_dresult* merged, const ptx_dinput_ops* in, ptx_dbatch** made, uint32_t* status_out);
ptx_status ptx_view_replace_plan_device(ptx_ctx* ctx, const ptx_dview* v, const uint16_t* pattern, uint32_t n_pattern, uint32_t flags, const uint32_t* replacement,
                                        uint32_t n_replacement, uint32_t n_batch_logs, const uint32_t* actor /* host, [n_batch_logs] */, uint32_t max_actors,
                                        ptx_replace_plan* counts, ptx_dinput_ops** ops);

/* Copy a resident batch back to the host (columns, envelope, headers; library-owned until ptx_host_batch_free). */
typedef struct ptx_host_batch {
    ptx_batch b;
    void* owner;
} ptx_host_batch;
ptx_status ptx_batch_download(ptx_ctx* ctx, const ptx_dbatch* b, ptx_host_batch* out);
void ptx_host_batch_free(ptx_host_batch* hb);

/* ---- introspection ---- */
/* Largest number of ops a log may have and still be merged ENTIRELY ON CHIP (the LDS kernel: one CU's 160 KB, 16-bit indices).  A longer log — the
 * reference has no bound, micromerge.ts:614-672 — is merged in the same ptx_merge call by the HBM-staged kernel (working set in device scratch the
 * library sizes per log, 32-bit indices; an order of magnitude slower per op), up to 2^26 rows and an id keyspace (max counter + 1) x (actors) of 2^30;
 * PTX_ERR_CAPACITY beyond that.  The editor-facing entry points follow (rounds 5-6): ptx_resolve_cursors on a log of any length; ptx_change too (its element list in
 * global scratch where one CU's LDS cannot hold it); ptx_replay_patches too (a log whose replay state does not fit one CU's LDS is replayed with that state
 * in global scratch, ptx_patches.reserved counts them; comment ops and comment ids of one log stay within 16-bit indices — 65 534 ops, 65 535 ids —,
 * PTX_ERR_CAPACITY for a log beyond that). */
uint32_t ptx_max_ops_per_log(const ptx_ctx* ctx);
/* Name of the kernel the merge launches (to find it in a rocprofv3 trace): the family's ... */
const char* ptx_kernel_name(void);
/* ... and the build of it ptx_merge launches for THIS resident batch under this context: "ptx_merge_kernel", "ptx_merge_kernel_w7" (the same body held to the
 * scalar registers of seven waves per SIMD: launched when the batch's LDS window lets more than 24 waves share a CU) or "ptx_merge_kernel_many" (admission of
 * documents with more than three actors); a split batch's few large logs run as "..._rest*" / "ptx_merge_big_kernel" beside it. */
const char* ptx_batch_kernel_name(const ptx_ctx* ctx, const ptx_dbatch* b);

#ifdef __cplusplus
}
#endif
#endif /* PERITEXT_HIP_H */
