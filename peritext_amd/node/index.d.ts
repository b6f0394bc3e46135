/**
 * Types of the MI355X batch merge engine's TypeScript/JS host.  The hot-path types are the reference's own
 * (reference/src/micromerge.ts:25-71,:133-212; src/peritext.ts:17-65,:35-38,:125-137): a maintainer can import
 * them from the reference instead — they are restated here so that the package type-checks on its own.
 */
export type ActorId = string
export type OperationId = string /** `${counter}@${actorId}` (micromerge.ts:35) */
export type Clock = Record<ActorId, number>
export type MarkType = "strong" | "em" | "comment" | "link"

export type BoundaryPosition =
    | { type: "before"; elemId: OperationId }
    | { type: "after"; elemId: OperationId }
    | { type: "startOfText" }
    | { type: "endOfText" }

export interface InsertOperation { opId: OperationId; action: "set"; obj: OperationId; elemId?: OperationId | "_head"; insert: true; value: string }
export interface DeleteOperation { opId: OperationId; action: "del"; obj: OperationId; elemId: OperationId }
export interface MakeListOperation { opId: OperationId; action: "makeList"; obj?: OperationId | "_root"; key: string }
export interface AddMarkOperation { opId: OperationId; action: "addMark"; obj: OperationId; start: BoundaryPosition; end: BoundaryPosition; markType: MarkType; attrs?: { url?: string; id?: string } }
export interface RemoveMarkOperation { opId: OperationId; action: "removeMark"; obj: OperationId; start: BoundaryPosition; end: BoundaryPosition; markType: MarkType; attrs?: { id?: string } }
export type Operation = InsertOperation | DeleteOperation | MakeListOperation | AddMarkOperation | RemoveMarkOperation | { opId: OperationId; action: string; [k: string]: unknown }

/** micromerge.ts:133-148 — what Micromerge.change(ops) takes: index-based operations on the text list (the only path this host serves) */
export type InputOperation =
    | { path: []; action: "makeList"; key: "text" }
    /** on a map object — the root map (path []) or a map nested in it (path = the keys down from the root), micromerge.ts:109-131 */
    | { path: string[]; action: "makeMap" | "makeList"; key: string }
    | { path: string[]; action: "set"; key: string; value: JsonValue }
    | { path: string[]; action: "del"; key: string }
    | { path: ["text"]; action: "insert"; index: number; values: string[] }
    | { path: ["text"]; action: "delete"; index: number; count: number }
    | { path: ["text"]; action: "addMark"; startIndex: number; endIndex: number; markType: MarkType; attrs?: { url?: string; id?: string } }
    | { path: ["text"]; action: "removeMark"; startIndex: number; endIndex: number; markType: MarkType; attrs?: { id?: string } }

/** micromerge.ts:60-71 */
export interface Change { actor: ActorId; seq: number; deps: Clock; startOp: number; ops: Operation[] }

export type MarkMap = { strong?: { active: true }; em?: { active: true }; link?: { url: string }; comment?: Array<{ id: string }> }
/** peritext.ts:35-38 */
export interface FormatSpanWithText { text: string; marks: MarkMap }

/** SoA op log of include/peritext_hip.h (one row per internal Operation, 32 bytes) + decode tables. */
export interface WireBatch {
    nLogs: number; nOps: number
    logOff: BigUint64Array; opId: BigUint64Array; refA: BigUint64Array; refB: BigUint64Array
    payload: Uint32Array; action: Uint8Array; markType: Uint8Array; sideA: Uint8Array; sideB: Uint8Array
    logHdr?: Uint32Array
    /** Change envelope (micromerge.ts:60-71) -> applyChange's causal admission runs on the device */
    chgOff?: BigUint64Array; maxActors?: number
    /** what the device reads: chgHdr = actorRank << 20 | nops, chgEnv rows of ((1 + maxActors + 3) & ~3) u16 = seq, deps[...] */
    chgHdr?: Uint32Array; chgEnv?: Uint16Array
    /** the wide envelope column (ptx_batch.chg_env_hi): high halves of chgEnv's values, present once some seq / dep exceeds 65534 */
    chgEnvHi?: Uint16Array
    /** the same unpacked (filled by encodeDocs / unpackEnvelope; decodeChanges and decodePatches read these) */
    chgActor?: Uint32Array; chgSeq?: Uint32Array; chgNops?: Uint32Array; chgDeps?: Uint32Array
    values: string[]; urls: string[]; logDoc: number[]; docActors: string[][]; docComments: string[][]
    /** keys of the map objects (ref_b of the PTX_ACT_MAPSET / MAPDEL / MAKELIST rows) and the JSON text of the values they set (payload) */
    keys?: string[]; mapValues?: string[]
    /** encodeDocs(listKeys): device log l merges the list under root key logList[l] ("a.b": the list under key b of the map under root key a — an OperationPath) of replica logReplica[l] of its document */
    logList?: string[]; logReplica?: number[]
}
export interface WireResult {
    logs: Uint32Array; values: Uint32Array; spans: Uint32Array; cintervals: Uint32Array; elemRank?: Uint32Array
    /** ABI 7: the rows are compact — log l's values at values[valueOff[l] .. valueOff[l + 1]), span rows (2 u32 each) from spanOff[l], comment intervals (3 u32 each) from cintOff[l] */
    valueOff: BigUint64Array; spanOff: BigUint64Array; cintOff: BigUint64Array
    /** with applyMaterialize(batch, true): ptx_patches (patch_off, {status, n_patches} per log, 4 u32 per record) */
    patchOff?: BigUint64Array; patchLogs?: Uint32Array; patches?: Uint32Array
}

/** micromerge.ts:214-222 — what applyChange returns (the makeList patch, the raw op upstream, is {action: "makeList"}) */
export type Patch =
    | { action: "makeList" }
    | { path: ["text"]; action: "insert"; index: number; values: string[]; marks: MarkMap }
    | { path: ["text"]; action: "delete"; index: number; count: number }
    | { path: ["text"]; action: "addMark"; markType: MarkType; startIndex: number; endIndex: number; attrs?: { url?: string; id?: string } }
    | { path: ["text"]; action: "removeMark"; markType: MarkType; startIndex: number; endIndex: number }

/** the columns of ptx_input_ops (include/peritext_hip.h) */
export interface WireInputOps {
    chgOff: BigUint64Array; opOff: BigUint64Array; action: Uint8Array; markType: Uint8Array
    index: Uint32Array; count: Uint32Array; payload: Uint32Array; values: Uint32Array; actor: Uint32Array; maxActors: number
}

/** Per-replica handle with the reference's calls (Micromerge.applyChange :499, change :308, getTextWithFormatting :516). */
export interface ReplicaHandle {
    /** causal admission (seq / deps) is checked HERE: throws RangeError like micromerge.ts:501-509 and leaves the replica untouched;
     *  the change itself is queued (all handles of an engine are merged in one launch); returns [] — see getPatches() */
    applyChange(change: Change): Patch[]
    /** Micromerge.change (micromerge.ts:308): InputOperations resolved against this replica's state on the device (ptx_change);
     *  throws RangeError("List index out of bounds") like :804.  Needs engine.replica(docId, actorId). */
    change(ops: InputOperation[]): { change: Change; patches: Patch[] }
    /** micromerge.ts:465-477, resolved on the device (ptx_resolve_cursors); RangeError like :804 / :752 */
    getCursor(path: ["text"], index: number): { objectId: OperationId | null; elemId: OperationId }
    resolveCursor(cursor: { objectId?: OperationId | null; elemId: OperationId }): number
    /** entry c = the Patch[] the reference's applyChange(c-th change) returns; a document of any length (beyond about 80 000 list elements the replay keeps its
     *  state in device memory instead of on chip: slower per op, the same patches) */
    getPatches(): Patch[][]
    /** throws RangeError("List element not found" | …) exactly where the reference's applyChange would have thrown */
    getTextWithFormatting(path: ["text"]): FormatSpanWithText[]
    /** Micromerge.getRoot() (micromerge.ts:443-449): the root map and the maps nested in it, resolved on the device (ptx_root_map: last
     *  writer wins per key, :572-602); list objects appear as { $list: true }.  RangeError("Object does not exist") like :538-540 */
    getRoot(): RootJson
}
/** a map object as JSON: nested maps, the values set, { $list: true } where a list object (the text) hangs */
export type RootJson = { [key: string]: RootJson | JsonValue | { $list: true } }
export type JsonValue = string | number | boolean | null | JsonValue[] | { [key: string]: JsonValue }
/** ptx_root_map's raw answer (include/peritext_hip.h ptx_root_maps) */
export interface WireRootMaps { entryOff: BigUint64Array; logs: Uint32Array; entries: Uint32Array }

export interface Snippet { log: number; hitStart: number; hitEnd: number; text: string; matchUnit: number; spans: FormatSpanWithText[] }
export interface TextView {
    findText(needle: string, opts?: { ignoreAsciiCase?: boolean; maxHits?: number }): Array<Array<{ status: number; count: number; hits: Array<{ unit: number; startIndex: number; endIndex: number }> }>>
    textSlices(ranges: Array<Array<Array<{ startIndex: number; endIndex: number }>>>): Array<Array<Array<{ status: number; startIndex: number; endIndex: number; spans: FormatSpanWithText[] }>>>
    findSnippets(needle: string, opts?: { ignoreAsciiCase?: boolean; maxHits?: number; before?: number; after?: number }): Array<Array<{ status: number; count: number; snippets: Snippet[] }>>
    /** replace all as change() input, planned on the device (ptx_view_replace_plan): the leftmost non-overlapping matches that cover whole elements, in
     *  descending order, a delete and an insert of replacement.split("") each; calls for changeMany = plan.map(logs => logs.map(x => (x.ops.length ? [x.ops] : []))) */
    replacePlan(needle: string, replacement: string, opts?: { asciiNocase?: boolean }): Array<Array<ReplacePlanOfLog>>
    /** the runs of a mark, chosen on the device (ptx_view_mark_runs): adjacent spans that carry it — for a link: with the same url — are one run; comment runs
     *  come per id.  A url or id a document does not have gives no runs.  count counts all runs, opts.maxRuns caps the listed ones */
    markRuns(sel: MarkSelector, opts?: { maxRuns?: number }): Array<Array<{ status: number; count: number; runs: MarkRun[] }>>
    /** markRuns and, per listed run, its text and formatting with opts.before / opts.after elements of context, in one device call (ptx_view_mark_snippets) */
    markSnippets(sel: MarkSelector, opts?: { maxRuns?: number; before?: number; after?: number }): Array<Array<{ status: number; count: number; snippets: MarkSnippet[] }>>
    /** findText restricted to the hits whose elements lie inside one run of `sel` (ptx_view_find_in_marks); a comment selector needs an id */
    findInMarks(needle: string, sel: MarkSelector, opts?: { ignoreAsciiCase?: boolean; maxHits?: number }): Array<Array<{ status: number; count: number; hits: Array<{ unit: number; startIndex: number; endIndex: number }> }>>
    free(): void
}
export type MarkSelector = { type: "strong" | "em" } | { type: "link"; url?: string } | { type: "comment"; id?: string }
/** [start, end): visible element indexes; unit / length: where the run's text sits in the replica's text (UTF-16 code units) */
export interface MarkRun { log: number; start: number; end: number; url?: string; id?: string; unit: number; length: number }
/** text.substr(matchUnit, length) is the run's own text */
export interface MarkSnippet extends MarkRun { text: string; spans: FormatSpanWithText[]; matchUnit: number }
export interface ReplacePlanOfLog {
    log: number
    /** the replica's merge / text status, or 5 (PTX_ERR_CAPACITY) where the Change would make more than 65 534 ops: then `ops` is empty */
    status: number
    nMatches: number
    nChosen: number
    nReplaced: number
    ops: InputOperation[]
}
export class MergeEngine {
    /** resident (default true): the logs of a document's replica() handles stay in HBM between calls — a read encodes and uploads only the Changes that
     *  arrived since (ptx_batch_append), merges the resident logs and fetches the Patch[] records of the new rows only (ptx_replay_patches_from).
     *  false: every read encodes, uploads and replays the whole log of every handle. */
    constructor(opts?: { device?: number; libPath?: string; addonPath?: string; resident?: boolean })
    /** what the resident replicas cost so far: documents uploaded whole (first read, or a new actor re-ranked its op ids), appends, rows sent to the device */
    readonly stats: { residentUploads: number; residentAppends: number; rowsUploaded: number; residentChanges: number; residentChangeMs: number; residentCursorCalls: number }
    close(): void
    applyMaterialize(batch: WireBatch, wantPatches?: boolean): WireResult
    /** docs -> replica logs -> changes in application order  =>  spans per replica log */
    /** without opts: the spans of the list under "text" per replica; with opts.listKeys (several list objects per document, round 5): every replica's entry is
     *  {key: getTextWithFormatting([key])} for the root keys named */
    applyChanges(docs: Change[][][], opts?: { listKeys?: string[]; text?: "device" | "host" }): FormatSpanWithText[][][] | Array<Array<{ [key: string]: FormatSpanWithText[] }>>
    /** every position of `needle` in every replica's text, found on the device without downloading the text (ptx_result_find_text): indexOf repeated from p + 1 over UTF-16
     *  code units; count = all matches, hits = the first opts.maxHits (default: all), ascending; [startIndex, endIndex) is the visible element range change() takes */
    findText(docs: Change[][][], needle: string, opts?: { ignoreAsciiCase?: boolean; maxHits?: number }): Array<Array<{ status: number; count: number; hits: Array<{ unit: number; startIndex: number; endIndex: number }> }>>
    /** the text, with its formatting, of element ranges of every replica, cut on the device without downloading the documents' text (ptx_result_text_slices):
     *  Array.prototype.slice's clamping for non-negative indexes; a replica's ranges may come in any order, overlap and repeat; per range, in that order, the range
     *  after clamping and the FormatSpanWithText[] of its elements */
    textSlices(docs: Change[][][], ranges: Array<Array<Array<{ startIndex: number; endIndex: number }>>>, opts?: {}): Array<Array<Array<{ status: number; startIndex: number; endIndex: number; spans: FormatSpanWithText[] }>>>
    /** A resident text view of every replica of `docs` (ptx_text_view_create): merged once, the text and the element prefix stay on the device; search and cut any
     *  number of times, then free().  findText and textSlices return what the engine's methods of the same name return; findSnippets finds and cuts in one device
     *  call: per listed hit the elements [hitStart - before, hitEnd + after), `text.substr(matchUnit, needle.length)` being the match. */
    textView(docs: Change[][][]): TextView
    /** spans as applyChanges + patches[doc][replica][change] = what applyChange(change) returns (micromerge.ts:499) */
    applyChangesWithPatches(docs: Change[][][]): { spans: FormatSpanWithText[][][]; patches: Patch[][][][] }
    /** patch streams (patchOff / patchLogs / patches of `res`: this library's, or a peer's) back into the documents they describe (ptx_accumulate_patches) */
    accumulatePatches(batch: WireBatch, res: { patchOff: BigUint64Array; patchLogs: Uint32Array; patches: Uint32Array }): WireResult
    /** the fuzzer's patch assertion on the device (ptx_check_patches): status[doc][replica], agrees[doc][replica], disagree = streams that do not rebuild their merged document */
    checkPatches(docs: Change[][][]): { status: number[][]; agrees: boolean[][]; disagree: number }
    /** getRoot() of every replica: roots[doc][replica] (ptx_root_map) */
    roots(docs: Change[][][]): RootJson[][]
    /** on-device change(): edit histories generated on the GPU (ptx_generate; the documents of oracle/ptxgen.js for the same seed) and merged there */
    generate(cfg: { replicas: number; opsPerLog: number; mix: [number, number, number, number]; markTypes: MarkType[]; seed: number; nDocs: number; firstDoc?: number; listCap?: number; initialText?: string }):
        { docs: Change[][][]; spans: FormatSpanWithText[][][]; kernelMs: number; batch: WireBatch }
    digests(docs: Change[][][]): Array<[bigint, bigint]>
    /** multi-GPU, one process per GPU: RCCL communicator (id made on rank 0, carried by the host's own channel) */
    commUniqueId(): Uint8Array
    commInit(id: Uint8Array, rank: number, nRanks: number): unknown
    commDestroy(comm: unknown): void
    /** merge this rank's documents, all-gather the digests of all ranks on the device (ptx_allgather_digests), count the converged documents of the job */
    convergedDocs(docs: Change[][][], comm: unknown, counts: number[], replicas: number): { converged: number; total: number; digests: Array<[bigint, bigint]>; statuses: number[] }
    /** Micromerge.change for many replicas in one call: calls[d][r] = change() calls of replica r of document d */
    changeMany(docs: Change[][][], calls: InputOperation[][][][], actors: ActorId[][], opts?: { extraComments?: string[][] }): { changes: Change[][][]; status: number[][] }
    /** getMissingChanges + applyChanges (test/merge.ts:4-38) for many replica pairs in one call (ptx_sync_replicas): per pair what `to` lacks, in the order it admits it */
    syncMany(docs: Change[][][], pairs: Array<{ doc: number; from: number; to: number }>, opts?: { maxAttempts?: number }): { changes: Change[][]; status: number[] }
    /** documents at past versions, many cuts in one call (ptx_batch_at_versions): per cut the spans at the version, its effective clock and — opts.diff — the Patch[] from there to the replica's present;
     *  a clock no replica could have had is status 3 with spans null */
    documentsAt(docs: Change[][][], cuts: Array<{ doc: number; replica: number; clock: Record<ActorId, number> }> | Array<{ doc: number; replica: number; changes: number }>, opts?: { diff?: boolean; text?: "device" | "host" }): Array<{ status: number; clock: Record<ActorId, number>; spans: FormatSpanWithText[] | null; patches?: Patch[] | null }>
    replica(docId?: number | string, actorId?: ActorId): ReplicaHandle
    flush(wantPatches?: boolean): void
}
export function encodeDocs(docs: Change[][][], opts?: { extraActors?: ActorId[][]; extraComments?: string[][]; textObjs?: Array<OperationId | null>; listKeys?: string[] }): WireBatch
export function encodeInputOps(batch: WireBatch, perLog: InputOperation[][][], actors: ActorId[]): WireInputOps
export function packEnvelope(batch: WireBatch): WireBatch
export function unpackEnvelope(batch: WireBatch): WireBatch
export function decodeSpans(batch: WireBatch, res: WireResult, log: number): FormatSpanWithText[]
export function decodePatches(batch: WireBatch, res: WireResult, log: number): Patch[][]
export function decodeChanges(batch: WireBatch, log: number, textObjOfLog?: OperationId | null): Change[]
export function decodeRoot(batch: WireBatch, rm: WireRootMaps, log: number): RootJson
/** bridge.ts:394-414 prosemirrorDocFromCRDT, as the Node.toJSON() form of the document (parity unpinned: no ProseMirror in the build image) */
export function prosemirrorDocFromSpans(spans: FormatSpanWithText[]): { type: "doc"; content: Array<{ type: "paragraph"; content?: Array<{ type: "text"; text: string; marks?: Array<{ type: MarkType; attrs?: Record<string, string> }> }> }> }
export function census(batch: WireBatch): Uint32Array
/** PTX_VERSION_ALL: a clock entry of documentsAt that keeps every change of the actor */
export const VERSION_ALL: number
