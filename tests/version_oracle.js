"use strict"
/*
 * TEST INFRASTRUCTURE: what the reference shows for a replica log at a past version, from the oracle and its harness as they are.
 *
 *   node tests/version_oracle.js IN.json OUT.json
 *   IN  = {logs: [Change[]], cuts: [{log: index into logs, clock: {actorId: seq | "all"}} | {log, changes: k}], thenRest: bool}
 *   OUT = {cuts: [{kept: [[actor, seq]], rest: [[actor, seq]], keptRows, error: null | {kind, message, at}, clock: {actorId: seq},
 *                  atVersion: {spans, text} | null, root, atEnd: {spans, text} | null, restPatches: Patch[] | null}]}
 *
 * Per cut the kept list is chosen HERE, from the definition: a change is kept iff seq <= clock[actor] (an absent actor is 0: merge.ts:30 `=== undefined`;
 * "all" keeps every change of the actor), or it is one of the first k of the log.  The kept changes are applied, in log order, to a fresh Micromerge with
 * the oracle's own applyChange; the first error stops the cut (`error.at` = the position in the kept list, `kind` = the first two words of its message).  With
 * thenRest the others follow, also in log order, and their concatenated applyChange returns are `restPatches`: the Patch[] from the version to the present.
 * `clock` is the fresh document's clock after the kept part, `root` its getRoot() with the lists as markers (oracle/cli.js rootOf), `atVersion` / `atEnd`
 * getTextWithFormatting(["text"]) after the kept part / at the end (null where the replica holds no text list yet).
 */
const fs = require("fs")
const path = require("path")
const O = require(path.join(__dirname, "..", "oracle", "peritext_oracle.js"))
require(path.join(__dirname, "..", "oracle", "harness.js"))

const key = c => [c.actor, c.seq]

function rootOf(v) {
    if (Array.isArray(v)) return { $list: true }
    if (v && typeof v === "object") {
        const o = {}
        for (const k of Object.keys(v)) o[k] = rootOf(v[k])
        return o
    }
    return v
}

/* the RangeError's first two words: "Missing dependency", "Expected sequence", "List element", ... */
const kindOf = e => String(e.message).replace(/[:,]/g, "").split(" ").slice(0, 2).join(" ")

function shown(doc) {
    if (!Array.isArray(doc.root.text)) return null
    return { spans: doc.getTextWithFormatting(["text"]), text: doc.root.text.slice() }
}

function runCut(logs, cut, thenRest) {
    const log = logs[cut.log]
    const keep =
        cut.clock !== undefined
            ? c => (cut.clock[c.actor] === "all" ? true : c.seq <= (cut.clock[c.actor] || 0))
            : (c, i) => i < cut.changes
    const kept = log.filter(keep)
    const rest = log.filter((c, i) => !keep(c, i))
    const out = { kept: kept.map(key), rest: rest.map(key), keptRows: kept.reduce((a, c) => a + c.ops.length, 0), error: null, clock: {}, atVersion: null, root: null, atEnd: null, restPatches: null }
    const doc = new O.Micromerge("version-reader")
    for (let i = 0; i < kept.length; i++) {
        try {
            doc.applyChange(O.normalizeChange(kept[i]))
        } catch (e) {
            out.error = { kind: kindOf(e), message: (e instanceof RangeError ? "RangeError: " : "Error: ") + e.message, at: i }
            return out
        }
    }
    out.clock = Object.assign({}, doc.clock)
    out.atVersion = shown(doc)
    out.root = rootOf(doc.root)
    if (thenRest) {
        const patches = []
        for (let i = 0; i < rest.length; i++) {
            try {
                for (const p of doc.applyChange(O.normalizeChange(rest[i]))) patches.push(p.action === "makeList" ? { action: "makeList" } : p)
            } catch (e) {
                out.error = { kind: kindOf(e), message: (e instanceof RangeError ? "RangeError: " : "Error: ") + e.message, at: kept.length + i }
                return out
            }
        }
        out.restPatches = patches
        out.atEnd = shown(doc)
    }
    return out
}

const input = JSON.parse(fs.readFileSync(process.argv[2], "utf8"))
fs.writeFileSync(process.argv[3], JSON.stringify({ cuts: input.cuts.map(c => runCut(input.logs, c, !!input.thenRest)) }))
