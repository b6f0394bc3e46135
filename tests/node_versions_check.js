/*
 * GPU check of MergeEngine.documentsAt (tests/test_node_versions.py runs it):
 *   node tests/node_versions_check.js IN.json
 *   IN = {docs: Change[][][], clockCuts: [{doc, replica, clock}], prefixCuts: [{doc, replica, changes}],
 *         expected: {clock: [...], prefix: [...]} per cut {status, clock, spans, patches}}   the oracle's answers (tests/version_oracle.js)
 * Every cut's status, effective clock and spans must be the oracle's, with and without diff; with diff the patches too.  A failed cut has no spans; bad
 * arguments throw.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const inp = JSON.parse(fs.readFileSync(process.argv[2], "utf8"))
const engine = new host.MergeEngine()
const sorted = v => JSON.parse(JSON.stringify(v, (k, x) => (x && typeof x === "object" && !Array.isArray(x) ? Object.keys(x).sort().reduce((o, key) => ((o[key] = x[key]), o), {}) : x)))
let checked = 0, failed = 0, patches = 0
for (const [kind, cuts] of [["clock", inp.clockCuts], ["prefix", inp.prefixCuts]]) {
    const want = inp.expected[kind]
    for (const diff of [false, true]) {
        const got = engine.documentsAt(inp.docs, cuts, { diff })
        assert.strictEqual(got.length, cuts.length)
        cuts.forEach((c, k) => {
            const what = kind + " cut " + k + (diff ? " (diff)" : "")
            assert.strictEqual(got[k].status, want[k].status, what + ": status")
            if (want[k].status !== 0) {
                assert.strictEqual(got[k].spans, null, what + ": a failed cut has no spans")
                assert.deepStrictEqual(got[k].clock, {})
                if (diff) assert.strictEqual(got[k].patches, null)
                failed += diff ? 0 : 1
                return
            }
            assert.deepStrictEqual(got[k].clock, want[k].clock, what + ": effective clock")
            assert.deepStrictEqual(sorted(got[k].spans), sorted(want[k].spans), what + ": spans at the version")
            assert.strictEqual("patches" in got[k], diff)
            if (diff) {
                assert.deepStrictEqual(sorted(got[k].patches), sorted(want[k].patches), what + ": patches from the version to the present")
                patches += got[k].patches.length
            }
            checked++
        })
    }
}
assert.deepStrictEqual(engine.documentsAt(inp.docs, []), [])
assert.throws(() => engine.documentsAt(inp.docs, [inp.clockCuts[0], inp.prefixCuts[0]]), /every cut carries/)
assert.throws(() => engine.documentsAt(inp.docs, [{ doc: 0, replica: 0 }]), /every cut carries/)
assert.throws(() => engine.documentsAt(inp.docs, [{ doc: 0, replica: 99, changes: 1 }]), /no replica 99/)
assert.throws(() => engine.documentsAt(inp.docs, [{ doc: inp.docs.length, replica: 0, changes: 1 }]), /no replica/)
assert.strictEqual(host.STATUS_MESSAGES[3], "Missing dependency")
assert.strictEqual(host.VERSION_ALL, 0xffffffff)
engine.close()
console.log(JSON.stringify({ ok: true, checked, failed, patches }))
