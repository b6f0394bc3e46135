/*
 * GPU check of MergeEngine.syncMany (tests/test_node_sync.py runs it):
 *   node tests/node_sync_check.js IN.json
 *   IN = {docs: Change[][][], pairs: [{doc, from, to}], expected: [{applied: Change[], status}]}   the oracle's answers (tests/sync_oracle.js)
 * Every pair's Changes must be deep-equal to the oracle's `applied`, in admitted order; a replica named as `to` twice is refused.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const inp = JSON.parse(fs.readFileSync(process.argv[2], "utf8"))
const engine = new host.MergeEngine()
const got = engine.syncMany(inp.docs, inp.pairs)
assert.strictEqual(got.changes.length, inp.pairs.length)
let changes = 0
inp.pairs.forEach((p, k) => {
    assert.strictEqual(got.status[k], inp.expected[k].status, "pair " + k + " status")
    assert.deepStrictEqual(got.changes[k], inp.expected[k].applied, "pair " + k + ": Changes differ from the oracle's")
    changes += got.changes[k].length
})
const unbounded = engine.syncMany(inp.docs, inp.pairs, { maxAttempts: 0 })
assert.deepStrictEqual(unbounded.changes, got.changes)
assert.throws(() => engine.syncMany(inp.docs, [inp.pairs[0], inp.pairs[0]]), /target of two pairs/)
assert.strictEqual(host.STATUS_MESSAGES[8], "applyChanges did not converge")
engine.close()
console.log(JSON.stringify({ ok: true, pairs: inp.pairs.length, changes }))
