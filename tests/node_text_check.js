/*
 * MergeEngine.applyChanges / documentsAt with { text: "device" } (tests/test_node_text.py runs it):
 *   node tests/node_text_check.js mock IN.json   no GPU: a stand-in addon hands back the rows and the text tests/test_node_text.py computed with the CPU emulation for
 *                                                the batch both encoders produce (IN.result / IN.text; IN.values / IN.payload pin that it IS the same batch)
 *   node tests/node_text_check.js gpu IN.json    the real addon on the MI355X
 *   IN = {docs: Change[][][], expected: FormatSpanWithText[][][] (the reference's known answers / the oracle's spans / the hand-written surrogate literal), ...}
 * With the option the spans deep-equal the default path's and the expected ones; without it the addon's new entry points are never called; the string table
 * goes up once per encoded batch and is freed with it.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const mode = process.argv[2]
const inp = JSON.parse(fs.readFileSync(process.argv[3], "utf8"))
const sorted = v => JSON.parse(JSON.stringify(v, (k, x) => (x && typeof x === "object" && !Array.isArray(x) ? Object.keys(x).sort().reduce((o, key) => ((o[key] = x[key]), o), {}) : x)))
/* a string as its UTF-16 code units: deepStrictEqual on strings would pass through JSON for lone surrogates, this does not */
const units = spans => spans.map(s => Array.from(s.text, (_, i) => s.text.charCodeAt(i)))
const sameSpans = (got, want, what) => {
    assert.deepStrictEqual(sorted(got), sorted(want), what)
    assert.deepStrictEqual(units(got), units(want), what + ": code units")
}

if (mode === "mock") {
    const calls = { applyMaterialize: 0, stringsUpload: 0, stringsFree: 0, resultText: 0 }
    const result = () => ({
        logs: Uint32Array.from(inp.result.logs), values: Uint32Array.from(inp.result.values), spans: Uint32Array.from(inp.result.spans), cintervals: Uint32Array.from(inp.result.cintervals),
        valueOff: BigUint64Array.from(inp.result.valueOff, BigInt), spanOff: BigUint64Array.from(inp.result.spanOff, BigInt), cintOff: BigUint64Array.from(inp.result.cintOff, BigInt),
    })
    const sameBatch = batch => {
        assert.deepStrictEqual(batch.values, inp.values, "the batch is the one the emulation merged")
        assert.deepStrictEqual(Array.from(batch.payload), inp.payload)
    }
    let live = null
    const mock = {
        open() {}, create() { return {} }, destroy() {},
        applyMaterialize(ctx, batch) { calls.applyMaterialize++; sameBatch(batch); return result() },
        stringsUpload(ctx, u, off) {
            calls.stringsUpload++
            assert.ok(u instanceof Uint16Array && off instanceof BigUint64Array && off.length === inp.values.length + 1 && Number(off[off.length - 1]) === u.length)
            /* the table is the batch's values as code units */
            inp.values.forEach((v, i) => assert.strictEqual(String.fromCharCode(...u.subarray(Number(off[i]), Number(off[i + 1]))), v))
            assert.strictEqual(live, null)
            live = { table: true }
            return live
        },
        stringsFree(ctx, h) { calls.stringsFree++; assert.strictEqual(h, live); live = null },
        resultText(ctx, batch, strings) {
            calls.resultText++
            sameBatch(batch)
            assert.strictEqual(strings, live, "the table is resident while the text is assembled")
            return Object.assign(result(), { text: Uint16Array.from(inp.text.text), textOff: BigUint64Array.from(inp.text.textOff, BigInt), textStatus: Uint32Array.from(inp.text.status),
                                             spanUnit: Uint32Array.from(inp.text.spanUnit) })
        },
    }
    const engine = new host.MergeEngine({ addon: mock })
    const plain = engine.applyChanges(inp.docs)
    assert.deepStrictEqual(calls, { applyMaterialize: 1, stringsUpload: 0, stringsFree: 0, resultText: 0 }, "without the option the new entry points are never called")
    assert.deepStrictEqual(engine.applyChanges(inp.docs, { text: "host" }), plain)
    assert.strictEqual(calls.stringsUpload + calls.resultText, 0)
    const dev = engine.applyChanges(inp.docs, { text: "device" })
    assert.deepStrictEqual(calls, { applyMaterialize: 2, stringsUpload: 1, stringsFree: 1, resultText: 1 }, "one upload per encoded batch, freed with it")
    assert.strictEqual(live, null)
    let checked = 0
    inp.docs.forEach((logs, d) => logs.forEach((_, r) => {
        sameSpans(dev[d][r], plain[d][r], "doc " + d + " replica " + r + ": device text against the default path")
        sameSpans(dev[d][r], inp.expected[d][r], "doc " + d + " replica " + r + ": against the expected spans")
        checked++
    }))
    assert.throws(() => engine.applyChanges(inp.docs, { text: "gpu" }), /"device" or "host"/)
    engine.close()
    console.log(JSON.stringify({ ok: true, checked }))
} else if (mode === "gpu") {
    const engine = new host.MergeEngine()
    const plain = engine.applyChanges(inp.docs), dev = engine.applyChanges(inp.docs, { text: "device" })
    let checked = 0
    inp.docs.forEach((logs, d) => logs.forEach((_, r) => {
        sameSpans(dev[d][r], plain[d][r], "doc " + d + " replica " + r + ": device text against the default path")
        sameSpans(dev[d][r], inp.expected[d][r], "doc " + d + " replica " + r + ": against the expected spans")
        checked++
    }))
    /* documentsAt: every replica at its first change, at half of its changes and at its present */
    const cuts = []
    inp.docs.forEach((logs, d) => logs.forEach((log, r) => { for (const k of [1, log.length >> 1, log.length]) cuts.push({ doc: d, replica: r, changes: k }) }))
    const a = engine.documentsAt(inp.docs, cuts), b = engine.documentsAt(inp.docs, cuts, { text: "device" })
    assert.strictEqual(a.length, cuts.length)
    let versions = 0
    cuts.forEach((c, k) => {
        assert.strictEqual(b[k].status, a[k].status)
        assert.deepStrictEqual(b[k].clock, a[k].clock)
        if (a[k].spans === null) assert.strictEqual(b[k].spans, null)
        else { sameSpans(b[k].spans, a[k].spans, "cut " + k); versions++ }
        if (c.changes === inp.docs[c.doc][c.replica].length) sameSpans(b[k].spans, inp.expected[c.doc][c.replica], "cut " + k + ": the present")
    })
    engine.close()
    console.log(JSON.stringify({ ok: true, checked, versions }))
} else {
    console.error("usage: node tests/node_text_check.js mock|gpu IN.json")
    process.exit(2)
}
