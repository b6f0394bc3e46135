/*
 * GPU check of MergeEngine.accumulatePatches / checkPatches (tests/test_node_accum.py runs it):
 *   node tests/node_accum_check.js tests/golden/patches_mini.json
 * The patch streams applyMaterialize(batch, true) returns, accumulated on the device, must decode to the fixture's own spans (made by the reference); a
 * stream with a record out of bounds fails its own log only; checkPatches agrees on every replica.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const gen = JSON.parse(fs.readFileSync(process.argv[2], "utf8"))
const docs = gen.docs.map(d => d.logs)
const engine = new host.MergeEngine()
const batch = host.encodeDocs(docs)
const res = engine.applyMaterialize(batch, true)
const acc = engine.accumulatePatches(batch, res)
assert.strictEqual(acc.elemRank, undefined)
let log = 0
for (const d of gen.docs)
    for (const e of d.expected) {
        assert.strictEqual(acc.logs[12 * log], 0, "log " + log + " status")
        assert.deepStrictEqual(host.decodeSpans(batch, acc, log), e.spans, "log " + log + ": spans differ from the fixture's")
        for (const k of [2, 3, 4, 5, 8, 9, 10, 11]) assert.strictEqual(acc.logs[12 * log + k], res.logs[12 * log + k], "log " + log + " word " + k) /* counts and digest of the merge */
        log++
    }
/* a foreign stream with its last record out of bounds: that log alone fails, at that record */
const bad = { patchOff: res.patchOff, patchLogs: res.patchLogs, patches: Uint32Array.from(res.patches) }
const n0 = res.patchLogs[1], last = 4 * (Number(res.patchOff[0]) + n0 - 1)
bad.patches[last + 1] = host.PATCH.DELETE
bad.patches[last + 2] = 0x7fffffff
bad.patches[last + 3] = 1
const acc2 = engine.accumulatePatches(batch, bad)
assert.strictEqual(acc2.logs[0], 7)
assert.strictEqual(acc2.logs[7], n0 - 1)
for (let l = 1; l < log; l++) assert.strictEqual(acc2.logs[12 * l], 0)
const chk = engine.checkPatches(docs)
assert.strictEqual(chk.disagree, 0)
assert.ok(chk.status.every(d => d.every(s => s === 0)) && chk.agrees.every(d => d.every(a => a === true)))
assert.strictEqual(chk.status.length, docs.length)
engine.close()
console.log(JSON.stringify({ ok: true, logs: log }))
