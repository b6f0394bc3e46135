/*
 * GPU check of the JS host on a document whose replay state exceeds one CU's LDS (tests/test_gpu_replay_hbm.py runs it):
 *   node tests/node_replay_hbm_check.js <n_chars>
 * A replica handle receives ONE Change that types n_chars characters in order; getPatches() must return the makeList patch followed by n_chars inserts,
 * patch k at index k - 1 with the k-th character and no marks — what the reference's applyChange returns for it (micromerge.ts:499-514, :661-671).
 */
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const n = parseInt(process.argv[2] || "100000", 10)
const ops = [{ opId: "1@doc1", action: "makeList", obj: "_root", key: "text" }]
for (let i = 0; i < n; i++)
    ops.push({ opId: i + 2 + "@doc1", action: "set", obj: "1@doc1", elemId: i === 0 ? "_head" : i + 1 + "@doc1", insert: true, value: "abcdefghij"[i % 10] })
const change = { actor: "doc1", seq: 1, deps: {}, startOp: 1, ops }

const engine = new host.MergeEngine()
const rep = engine.replica(0)
assert.deepStrictEqual(rep.applyChange(change), [])
const got = rep.getPatches()
assert.strictEqual(got.length, 1, "one Patch[] per applied change")
const patches = got[0]
assert.strictEqual(patches.length, n + 1)
assert.deepStrictEqual(patches[0], { action: "makeList" })
for (let k = 1; k <= n; k++) {
    const p = patches[k]
    if (p.action !== "insert" || p.index !== k - 1 || p.values.length !== 1 || p.values[0] !== "abcdefghij"[(k - 1) % 10] || Object.keys(p.marks).length !== 0 ||
        p.path.length !== 1 || p.path[0] !== "text")
        assert.fail("patch " + k + ": " + JSON.stringify(p))
}
const text = rep.getTextWithFormatting(["text"])
assert.strictEqual(text.length, 1)
assert.strictEqual(text[0].text.length, n)
engine.close()
console.log(JSON.stringify({ ok: true, patches: patches.length }))
