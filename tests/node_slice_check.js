/*
 * MergeEngine.textSlices (tests/test_node_slices.py runs it):
 *   node tests/node_slice_check.js mock IN.json   no GPU: a stand-in addon hands back the slices tests/test_node_slices.py computed with the CPU emulation for the
 *                                                 batch both encoders produce (IN.slices; IN.values / IN.payload pin that it IS the same batch)
 *   node tests/node_slice_check.js gpu IN.json    the real addon on the MI355X
 *   IN = {docs: Change[][][], ranges: [[[{startIndex, endIndex}]]], expected: [[[{status, startIndex, endIndex, spans}]]] (the oracle's spans cut by a plain
 *   loop, element boundaries from the merge's value ids), whole: [[index of the range (0, 0xFFFFFFFF)]], ...}
 * Every range equals the expected one; the range that covers a whole replica returns the default path's spans; every other range's joined text is a stretch of
 * the default path's joined span texts; the string table goes up once per call and is freed with it.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const mode = process.argv[2]
const inp = JSON.parse(fs.readFileSync(process.argv[3], "utf8"))

function check(engine) {
    const plain = engine.applyChanges(inp.docs)
    const got = engine.textSlices(inp.docs, inp.ranges)
    let checked = 0, rows = 0
    assert.strictEqual(got.length, inp.docs.length)
    inp.docs.forEach((logs, d) => {
        assert.strictEqual(got[d].length, logs.length)
        logs.forEach((_, r) => {
            const what = "doc " + d + " replica " + r
            const text = plain[d][r].map(s => s.text).join("")
            assert.strictEqual(got[d][r].length, inp.ranges[d][r].length, what)
            got[d][r].forEach((s, j) => {
                assert.deepStrictEqual(s, inp.expected[d][r][j], what + " range " + j + ": against the oracle's spans cut to the range")
                assert.ok(text.includes(s.spans.map(x => x.text).join("")), what + " range " + j + ": a stretch of the default path's text")
                checked++
                rows += s.spans.length
            })
            assert.deepStrictEqual(got[d][r][inp.whole[d][r]].spans, plain[d][r], what + ": the whole replica as one range returns the default path's spans")
        })
    })
    assert.throws(() => engine.textSlices(inp.docs, []), /ranges/)
    assert.throws(() => engine.textSlices(inp.docs, inp.docs.map(logs => logs.map(() => [{ startIndex: -1, endIndex: 2 }]))), /unsigned/)
    return { checked, rows }
}

if (mode === "mock") {
    const calls = { applyMaterialize: 0, stringsUpload: 0, stringsFree: 0, textSlices: 0 }
    const sameBatch = batch => {
        assert.deepStrictEqual(batch.values, inp.values, "the batch is the one the emulation merged")
        assert.deepStrictEqual(Array.from(batch.payload), inp.payload)
    }
    const rows = () => ({
        logs: Uint32Array.from(inp.result.logs), values: Uint32Array.from(inp.result.values), spans: Uint32Array.from(inp.result.spans), cintervals: Uint32Array.from(inp.result.cintervals),
        valueOff: BigUint64Array.from(inp.result.valueOff, BigInt), spanOff: BigUint64Array.from(inp.result.spanOff, BigInt), cintOff: BigUint64Array.from(inp.result.cintOff, BigInt),
    })
    let live = null
    const mock = {
        open() {}, create() { return {} }, destroy() {},
        applyMaterialize(ctx, batch) {
            calls.applyMaterialize++
            sameBatch(batch)
            return rows()
        },
        stringsUpload(ctx, u, off) {
            calls.stringsUpload++
            assert.ok(u instanceof Uint16Array && off instanceof BigUint64Array && off.length === inp.values.length + 1 && Number(off[off.length - 1]) === u.length)
            assert.strictEqual(live, null)
            live = { table: true }
            return live
        },
        stringsFree(ctx, h) { calls.stringsFree++; assert.strictEqual(h, live); live = null },
        textSlices(ctx, batch, strings, off, start, end) {
            calls.textSlices++
            sameBatch(batch)
            assert.strictEqual(strings, live, "the table is resident while the slices are cut")
            assert.ok(off instanceof BigUint64Array && start instanceof Uint32Array && end instanceof Uint32Array)
            const m = inp.slices
            assert.deepStrictEqual(Array.from(off, Number), m.sliceOff, "the ranges arrive flat, in document-major order")
            assert.deepStrictEqual(Array.from(start), m.sliceStart)
            assert.deepStrictEqual(Array.from(end), m.sliceEnd)
            return Object.assign(rows(), { sliceStatus: Uint32Array.from(m.status), elemStart: Uint32Array.from(m.elemStart), elemEnd: Uint32Array.from(m.elemEnd),
                                           unitOff: BigUint64Array.from(m.unitOff, BigInt), sspanOff: BigUint64Array.from(m.sspanOff, BigInt), sliceText: Uint16Array.from(m.text),
                                           sspans: Uint32Array.from(m.sspans), sspanUnit: Uint32Array.from(m.sspanUnit), kernelMs: 0 })
        },
    }
    const engine = new host.MergeEngine({ addon: mock })
    const out = check(engine)
    assert.deepStrictEqual(calls, { applyMaterialize: 1, stringsUpload: 1, stringsFree: 1, textSlices: 1 }, "one upload per call, freed with it")
    assert.strictEqual(live, null)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else if (mode === "gpu") {
    const engine = new host.MergeEngine()
    const out = check(engine)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else {
    console.error("usage: node tests/node_slice_check.js mock|gpu IN.json")
    process.exit(2)
}
