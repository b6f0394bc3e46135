/*
 * MergeEngine.textView (tests/test_node_view.py runs it):
 *   node tests/node_view_check.js mock IN.json   no GPU: a stand-in addon hands back the answers tests/test_node_view.py computed with the CPU emulation of the
 *                                                view for the batch both encoders produce (IN.values / IN.payload pin that it IS the same batch)
 *   node tests/node_view_check.js gpu IN.json    the real addon on the MI355X
 *   IN = {docs: Change[][][], calls: [{needle, opts, expected: [[{status, count, snippets}]] (the oracle's text searched and its spans cut by plain loops)}], ...}
 * Every findSnippets answer equals the expected one, and, with no help from Python: its hits are indexOf repeated from p + 1 over the default path's joined
 * span texts (folded for ignoreAsciiCase), every snippet is a slice of that text which holds the needle at matchUnit, its spans join to it; findText and
 * textSlices of the same view return what the engine's own findText and textSlices return; one view serves every call and is freed once.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const mode = process.argv[2]
const inp = JSON.parse(fs.readFileSync(process.argv[3], "utf8"))
const fold = s => s.replace(/[A-Z]/g, c => c.toLowerCase()) /* ASCII only, as PTX_FIND_ASCII_NOCASE */

function check(engine, twins) {
    const plain = engine.applyChanges(inp.docs)
    const view = engine.textView(inp.docs)
    let snippets = 0, rows = 0
    for (const call of inp.calls) {
        const got = view.findSnippets(call.needle, call.opts)
        assert.deepStrictEqual(got, call.expected, "findSnippets " + JSON.stringify(call.needle) + ": against the oracle's text searched and cut by plain loops")
        const nocase = !!call.opts.ignoreAsciiCase, cap = call.opts.maxHits === undefined ? Infinity : call.opts.maxHits
        const needle = nocase ? fold(call.needle) : call.needle
        let log = 0
        inp.docs.forEach((logs, d) => logs.forEach((_, r) => {
            const what = "doc " + d + " replica " + r + " needle " + JSON.stringify(call.needle)
            const text = plain[d][r].map(s => s.text).join(""), hay = nocase ? fold(text) : text
            const at = []
            for (let p = hay.indexOf(needle); p >= 0; p = hay.indexOf(needle, p + 1)) at.push(p)
            assert.strictEqual(got[d][r].count, at.length, what + ": indexOf repeated from p + 1")
            assert.strictEqual(got[d][r].snippets.length, Math.min(at.length, cap), what)
            got[d][r].snippets.forEach((s, j) => {
                assert.strictEqual(s.log, log, what)
                assert.strictEqual(s.text, text.slice(at[j] - s.matchUnit, at[j] - s.matchUnit + s.text.length), what + " hit " + j + ": the snippet is a slice of the text around the hit")
                const m = s.text.substr(s.matchUnit, needle.length)
                assert.strictEqual(nocase ? fold(m) : m, needle, what + " hit " + j + ": the needle stands at matchUnit")
                assert.strictEqual(s.spans.map(x => x.text).join(""), s.text, what + " hit " + j + ": the spans join to the snippet")
                assert.ok(s.hitStart < s.hitEnd, what)
                snippets++
                rows += s.spans.length
            })
            log++
        }))
        if (twins) {
            assert.deepStrictEqual(view.findText(call.needle, call.opts), engine.findText(inp.docs, call.needle, call.opts), "view.findText is the engine's findText")
            const ranges = got.map(logs => logs.map(x => x.snippets.map(s => ({ startIndex: Math.max(s.hitStart - (call.opts.before || 0), 0), endIndex: Math.min(s.hitEnd + (call.opts.after || 0), 0xFFFFFFFF) }))))
            const cut = view.textSlices(ranges)
            assert.deepStrictEqual(cut, engine.textSlices(inp.docs, ranges), "view.textSlices is the engine's textSlices")
            got.forEach((logs, d) => logs.forEach((x, r) => x.snippets.forEach((s, j) => assert.deepStrictEqual(cut[d][r][j].spans, s.spans, "a snippet is the slice of its window"))))
        }
    }
    assert.throws(() => view.findSnippets("", {}), /needle/)
    assert.throws(() => view.findSnippets("a", { before: -1 }), /before/)
    assert.throws(() => view.textSlices([]), /ranges/)
    view.free()
    view.free()
    assert.throws(() => view.findSnippets("a", {}), /freed/)
    return { snippets, rows }
}

if (mode === "mock") {
    const calls = { applyMaterialize: 0, stringsUpload: 0, stringsFree: 0, viewCreate: 0, viewFindSnippets: 0, viewFree: 0 }
    const sameBatch = batch => {
        assert.deepStrictEqual(batch.values, inp.values, "the batch is the one the emulation merged")
        assert.deepStrictEqual(Array.from(batch.payload), inp.payload)
    }
    const big = a => BigUint64Array.from(a, BigInt)
    const rows = () => ({
        logs: Uint32Array.from(inp.result.logs), values: Uint32Array.from(inp.result.values), spans: Uint32Array.from(inp.result.spans), cintervals: Uint32Array.from(inp.result.cintervals),
        valueOff: big(inp.result.valueOff), spanOff: big(inp.result.spanOff), cintOff: big(inp.result.cintOff),
    })
    let strings = null, view = null
    const mock = {
        open() {}, create() { return {} }, destroy() {},
        applyMaterialize(ctx, batch) { calls.applyMaterialize++; sameBatch(batch); return rows() },
        stringsUpload() { calls.stringsUpload++; assert.strictEqual(strings, null); strings = { table: true }; return strings },
        stringsFree(ctx, h) { calls.stringsFree++; assert.strictEqual(h, strings); strings = null },
        viewCreate(ctx, batch, s) {
            calls.viewCreate++
            sameBatch(batch)
            assert.strictEqual(s, strings, "the table is resident while the view is made")
            view = { view: true }
            return Object.assign(rows(), { handle: view })
        },
        viewFindSnippets(ctx, h, pattern, flags, maxHits, before, after) {
            calls.viewFindSnippets++
            assert.strictEqual(h, view)
            assert.strictEqual(strings, null, "the table was freed after the creation: a query needs none")
            const needle = String.fromCharCode(...pattern)
            const call = inp.calls.find(c => c.needle === needle)
            assert.ok(call && pattern instanceof Uint16Array, "a needle of the test")
            assert.deepStrictEqual([flags, maxHits, before, after], [call.opts.ignoreAsciiCase ? 1 : 0, call.opts.maxHits === undefined ? 0xFFFFFFFF : call.opts.maxHits, call.opts.before || 0, call.opts.after || 0])
            const m = call.answer
            return { status: Uint32Array.from(m.status), nMatches: Uint32Array.from(m.nMatches), hitOff: big(m.hitOff), hitUnit: Uint32Array.from(m.hitUnit), hitStart: Uint32Array.from(m.hitStart),
                     hitEnd: Uint32Array.from(m.hitEnd), sliceStatus: Uint32Array.from(m.status), elemStart: Uint32Array.from(m.elemStart), elemEnd: Uint32Array.from(m.elemEnd), unitOff: big(m.unitOff),
                     sspanOff: big(m.sspanOff), sliceText: Uint16Array.from(m.text), sspans: Uint32Array.from(m.sspans), sspanUnit: Uint32Array.from(m.sspanUnit), matchUnit: Uint32Array.from(m.matchUnit), kernelMs: 0 }
        },
        viewFree(ctx, h) { calls.viewFree++; assert.strictEqual(h, view); view = null },
    }
    const engine = new host.MergeEngine({ addon: mock })
    const out = check(engine, false)
    assert.deepStrictEqual(calls, { applyMaterialize: 1, stringsUpload: 1, stringsFree: 1, viewCreate: 1, viewFindSnippets: inp.calls.length, viewFree: 1 }, "one view for every call, freed once")
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else if (mode === "gpu") {
    const engine = new host.MergeEngine()
    const out = check(engine, true)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else {
    console.error("usage: node tests/node_view_check.js mock|gpu IN.json")
    process.exit(2)
}
