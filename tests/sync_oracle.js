"use strict"
/*
 * TEST INFRASTRUCTURE: what the reference answers for a sync between two replicas (test/merge.ts:4-38), from the oracle and its harness as they are.
 *
 *   node tests/sync_oracle.js IN.json OUT.json
 *   IN  = {pairs: [{source: Change[], target: Change[]}]}   two logs of one document, in application order
 *   OUT = {pairs: [{missing: [[actor, seq]], applied: [[actor, seq]], threw: bool, attempts: T | null, twin: [[actor, seq]], stuck: bool, sourceInvalid: bool}]}
 *
 *   node tests/sync_oracle.js --session IN.json OUT.json
 *   IN  = {docs: D, replicas: R, text, rounds: [[{edit: {replica, ops: InputOperation[]} | null, sync: [left, right]} per document]]}
 *   OUT = {initial: Change, rounds: [[{made: Change | null, logs: [[[actor, seq]] per replica]} per document]]}
 * The multi-replica loop of test/fuzz.ts:165-199 for a given script: generateDocs, per round one change() and the two applyChanges(getMissingChanges())
 * calls of :198-199, in that order; `logs` = what every replica has applied so far, in application order.
 *
 * Per pair: `queues` per actor from the document's changes (test/fuzz.ts keeps them as the changes are made), both replicas rebuilt from their logs,
 * getMissingChanges(source, target) + applyChanges(target, missing, applied) of oracle/harness.js.  `attempts` / `twin` come from a guard-free twin of
 * that loop over the oracle's own applyChange on a second copy of the target: T = the attempts the loop makes without the 10 002-attempt guard (the
 * expectation for max_attempts = 0), null with stuck = true when a whole pass admits nothing (the reference would spin into its guard).
 * A source log no replica could have applied cannot be rebuilt with applyChange: getMissingChanges reads only its clock, which is then walked off the
 * log the way applyChange sets it (micromerge.ts:511), and sourceInvalid says so.
 */
const fs = require("fs")
const path = require("path")
const O = require(path.join(__dirname, "..", "oracle", "peritext_oracle.js"))
const H = require(path.join(__dirname, "..", "oracle", "harness.js"))

const key = c => [c.actor, c.seq]

function replica(log) {
    const doc = new O.Micromerge("sync-reader")
    for (const c of log) doc.applyChange(O.normalizeChange(c))
    return doc
}

function queuesOf(logs) {
    const seen = {}
    const queues = {}
    for (const log of logs) {
        for (const c of log) {
            const k = c.actor + "/" + c.seq
            if (seen[k]) continue
            seen[k] = true
            if (!queues[c.actor]) queues[c.actor] = []
            queues[c.actor].push(c)
        }
    }
    for (const a of Object.keys(queues)) {
        queues[a].sort((x, y) => x.seq - y.seq)
        /* getMissingChanges slices by seq: position k holds seq k + 1 (a hand-made source with a gap is padded so that the slices stay aligned) */
        const dense = []
        for (const c of queues[a]) dense[c.seq - 1] = c
        queues[a] = dense
    }
    return queues
}

function twinLoop(doc, changes) {
    const queue = changes.slice()
    const applied = []
    let attempts = 0
    let failedInARow = 0 /* every change of the queue has failed against the same state: nothing will ever change */
    while (queue.length > 0) {
        const c = queue.shift()
        attempts++
        try {
            doc.applyChange(c)
            applied.push(c)
            failedInARow = 0
        } catch (e) {
            queue.push(c)
            if (++failedInARow >= queue.length) return { attempts: null, applied, stuck: true }
        }
    }
    return { attempts, applied, stuck: false }
}

function runPair(p) {
    const queues = queuesOf([p.source, p.target])
    let source
    let sourceInvalid = false
    try {
        source = replica(p.source)
    } catch (e) {
        sourceInvalid = true
        source = { clock: {} }
        for (const c of p.source) source.clock[c.actor] = c.seq
    }
    const target = replica(p.target)
    const missing = H.getMissingChanges(source, target, queues).filter(c => c !== undefined).map(O.normalizeChange)
    const applied = []
    let threw = false
    try {
        H.applyChanges(target, missing, applied)
    } catch (e) {
        threw = true
    }
    const twin = twinLoop(replica(p.target), missing)
    return { missing: missing.map(key), applied: applied.map(key), threw, attempts: twin.attempts, twin: twin.applied.map(key), stuck: twin.stuck, sourceInvalid }
}

function runSession(inp) {
    const out = { initial: null, rounds: inp.rounds.map(() => []) }
    for (let d = 0; d < inp.docs; d++) {
        const g = H.generateDocs(inp.text, inp.replicas)
        out.initial = g.initialChange
        const queues = {}
        queues[g.initialChange.actor] = [g.initialChange]
        const logs = g.docs.map(() => [g.initialChange])
        inp.rounds.forEach((round, k) => {
            const step = round[d]
            let made = null
            if (step.edit) {
                const doc = g.docs[step.edit.replica]
                made = doc.change(step.edit.ops).change
                if (!queues[doc.actorId]) queues[doc.actorId] = []
                queues[doc.actorId].push(made)
                logs[step.edit.replica].push(made)
            }
            const left = step.sync[0]
            const right = step.sync[1]
            H.applyChanges(g.docs[right], H.getMissingChanges(g.docs[left], g.docs[right], queues), logs[right])
            H.applyChanges(g.docs[left], H.getMissingChanges(g.docs[right], g.docs[left], queues), logs[left])
            out.rounds[k].push({ made, logs: logs.map(l => l.map(key)) })
        })
    }
    return out
}

if (process.argv[2] === "--session") {
    fs.writeFileSync(process.argv[4], JSON.stringify(runSession(JSON.parse(fs.readFileSync(process.argv[3], "utf8")))))
} else {
    const input = JSON.parse(fs.readFileSync(process.argv[2], "utf8"))
    fs.writeFileSync(process.argv[3], JSON.stringify({ pairs: input.pairs.map(runPair) }))
}
