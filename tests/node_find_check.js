/*
 * MergeEngine.findText (tests/test_node_find.py runs it):
 *   node tests/node_find_check.js mock IN.json   no GPU: a stand-in addon hands back the matches tests/test_node_find.py computed with the CPU emulation for the
 *                                                batch both encoders produce (IN.queries[q].matches; IN.values / IN.payload pin that it IS the same batch)
 *   node tests/node_find_check.js gpu IN.json    the real addon on the MI355X
 *   IN = {docs: Change[][][], queries: [{needle, opts, expected: [[{status, count, hits}]] (a plain loop over the oracle's text, element boundaries from the
 *   merge's value ids), ...}], ...}
 * Every replica's count and hit units equal text.indexOf(needle, p + 1) repeated over the default path's joined span texts; the element ranges equal the
 * expected ones; the string table goes up once per call and is freed with it.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const mode = process.argv[2]
const inp = JSON.parse(fs.readFileSync(process.argv[3], "utf8"))
const foldAscii = s => s.replace(/[A-Z]/g, c => c.toLowerCase())
const positions = (text, needle, nocase) => {
    if (nocase) { text = foldAscii(text); needle = foldAscii(needle) }
    const out = []
    for (let p = text.indexOf(needle); p !== -1; p = text.indexOf(needle, p + 1)) out.push(p)
    return out
}

function check(engine) {
    const plain = engine.applyChanges(inp.docs)
    let checked = 0, hits = 0
    for (const q of inp.queries) {
        const got = engine.findText(inp.docs, q.needle, q.opts)
        const cap = q.opts && q.opts.maxHits !== undefined ? q.opts.maxHits : Infinity
        assert.strictEqual(got.length, inp.docs.length)
        inp.docs.forEach((logs, d) => {
            assert.strictEqual(got[d].length, logs.length)
            logs.forEach((_, r) => {
                const what = JSON.stringify(q.needle) + " doc " + d + " replica " + r
                const text = plain[d][r].map(s => s.text).join("")
                const want = positions(text, q.needle, q.opts && q.opts.ignoreAsciiCase)
                assert.strictEqual(got[d][r].status, 0, what)
                assert.strictEqual(got[d][r].count, want.length, what + ": count against indexOf")
                assert.deepStrictEqual(got[d][r].hits.map(h => h.unit), want.slice(0, cap), what + ": units against indexOf")
                assert.deepStrictEqual(got[d][r], q.expected[d][r], what + ": against the expected element ranges")
                checked++
                hits += got[d][r].hits.length
            })
        })
    }
    assert.throws(() => engine.findText(inp.docs, ""), /needle/)
    assert.throws(() => engine.findText(inp.docs, "a".repeat(257)), /needle/)
    assert.throws(() => engine.findText(inp.docs, "a", { maxHits: -1 }), /maxHits/)
    return { checked, hits }
}

if (mode === "mock") {
    const calls = { applyMaterialize: 0, stringsUpload: 0, stringsFree: 0, findText: 0 }
    const sameBatch = batch => {
        assert.deepStrictEqual(batch.values, inp.values, "the batch is the one the emulation merged")
        assert.deepStrictEqual(Array.from(batch.payload), inp.payload)
    }
    let live = null
    const mock = {
        open() {}, create() { return {} }, destroy() {},
        applyMaterialize(ctx, batch) {
            calls.applyMaterialize++
            sameBatch(batch)
            return {
                logs: Uint32Array.from(inp.result.logs), values: Uint32Array.from(inp.result.values), spans: Uint32Array.from(inp.result.spans), cintervals: Uint32Array.from(inp.result.cintervals),
                valueOff: BigUint64Array.from(inp.result.valueOff, BigInt), spanOff: BigUint64Array.from(inp.result.spanOff, BigInt), cintOff: BigUint64Array.from(inp.result.cintOff, BigInt),
            }
        },
        stringsUpload(ctx, u, off) {
            calls.stringsUpload++
            assert.ok(u instanceof Uint16Array && off instanceof BigUint64Array && off.length === inp.values.length + 1 && Number(off[off.length - 1]) === u.length)
            assert.strictEqual(live, null)
            live = { table: true }
            return live
        },
        stringsFree(ctx, h) { calls.stringsFree++; assert.strictEqual(h, live); live = null },
        findText(ctx, batch, strings, pattern, flags, maxHits) {
            calls.findText++
            sameBatch(batch)
            assert.strictEqual(strings, live, "the table is resident while the text is searched")
            assert.ok(pattern instanceof Uint16Array)
            const q = inp.queries.find(x => x.needle.length === pattern.length && Array.from(pattern).every((u, i) => u === x.needle.charCodeAt(i)) &&
                                            flags === (x.opts && x.opts.ignoreAsciiCase ? 1 : 0) && maxHits === (x.opts && x.opts.maxHits !== undefined ? x.opts.maxHits : 0xFFFFFFFF))
            assert.ok(q, "the needle arrives as its UTF-16 code units, the options as flags and cap")
            const m = q.matches
            return { status: Uint32Array.from(m.status), nMatches: Uint32Array.from(m.nMatches), hitOff: BigUint64Array.from(m.hitOff, BigInt), hitUnit: Uint32Array.from(m.hitUnit),
                     hitStart: Uint32Array.from(m.hitStart), hitEnd: Uint32Array.from(m.hitEnd), kernelMs: 0 }
        },
    }
    const engine = new host.MergeEngine({ addon: mock })
    const out = check(engine)
    assert.deepStrictEqual(calls, { applyMaterialize: 1, stringsUpload: inp.queries.length, stringsFree: inp.queries.length, findText: inp.queries.length }, "one upload per call, freed with it")
    assert.strictEqual(live, null)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else if (mode === "gpu") {
    const engine = new host.MergeEngine()
    const out = check(engine)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else {
    console.error("usage: node tests/node_find_check.js mock|gpu IN.json")
    process.exit(2)
}
