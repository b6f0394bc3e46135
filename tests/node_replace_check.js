/*
 * textView.replacePlan of MergeEngine (tests/test_node_replace.py runs it):
 *   node tests/node_replace_check.js mock IN.json   no GPU: a stand-in addon hands back the plans tests/test_node_replace.py computed with the CPU emulation for the
 *                                                   batch both encoders produce (IN.values / IN.payload pin that it IS the same batch)
 *   node tests/node_replace_check.js gpu IN.json    the real addon on the MI355X; changeMany with the plan's ops returns the oracle's Changes
 *   IN = {docs: Change[][][], firstEdge, oneUnit: boolean[][], calls: [{needle, replacement, opts, expected: [[{log, status, nMatches, nChosen, nReplaced, ops}]],
 *         expectedChanges?}], ...}
 * Every replacePlan answer deep-equals the expected one, and, with no help from Python: nMatches is indexOf repeated from p + 1 over the default path's joined span
 * texts (folded for asciiNocase), nChosen is the number of pieces split() cuts minus one, and where every element of a replica is one code unit (IN.oneUnit) the
 * ops applied to text.split("") by splice join to what a replaceAll loop makes of the text; one view serves every call and is freed once.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const mode = process.argv[2]
const inp = JSON.parse(fs.readFileSync(process.argv[3], "utf8"))
const fold = s => s.replace(/[A-Z]/g, c => c.toLowerCase()) /* ASCII only, as PTX_FIND_ASCII_NOCASE */

function replaceAllLoop(text, needle, replacement, nocase) {
    const hay = nocase ? fold(text) : text, n = nocase ? fold(needle) : needle
    let out = "", i = 0
    while (i < text.length) {
        if (hay.startsWith(n, i)) {
            out += replacement
            i += n.length
        } else out += text[i++]
    }
    return out
}

function check(engine, withChanges) {
    const plain = engine.applyChanges(inp.docs)
    const view = engine.textView(inp.docs)
    let replaced = 0, skipped = 0, changes = 0
    for (const call of inp.calls) {
        const got = view.replacePlan(call.needle, call.replacement, call.opts)
        assert.deepStrictEqual(got, call.expected, "replacePlan " + JSON.stringify(call.needle) + ": against the oracle's text searched, chosen and cut by plain loops")
        const nocase = !!call.opts.asciiNocase
        const needle = nocase ? fold(call.needle) : call.needle
        let log = 0
        inp.docs.forEach((logs, d) => logs.forEach((_, r) => {
            const what = "doc " + d + " replica " + r + " needle " + JSON.stringify(call.needle)
            const text = plain[d][r].map(s => s.text).join(""), hay = nocase ? fold(text) : text
            const g = got[d][r]
            let n = 0
            for (let p = hay.indexOf(needle); p >= 0; p = hay.indexOf(needle, p + 1)) n++
            assert.strictEqual(g.log, log++, what)
            assert.strictEqual(g.nMatches, n, what + ": indexOf repeated from p + 1")
            assert.strictEqual(g.nChosen, hay.split(needle).length - 1, what + ": the leftmost non-overlapping matches")
            assert.ok(g.nReplaced <= g.nChosen && g.ops.length === g.nReplaced * (call.replacement.length ? 2 : 1), what)
            if (inp.oneUnit[d][r]) {
                const elems = text.split("")
                for (const op of g.ops) {
                    if (op.action === "delete") elems.splice(op.index, op.count)
                    else elems.splice(op.index, 0, ...op.values)
                }
                assert.strictEqual(g.nReplaced, g.nChosen, what)
                assert.strictEqual(elems.join(""), replaceAllLoop(text, call.needle, call.replacement, nocase), what + ": the ops applied are replaceAll")
            }
            replaced += g.nReplaced
            skipped += g.nChosen - g.nReplaced
        }))
        if (withChanges) {
            const docs = inp.docs.slice(inp.firstEdge)
            const calls = got.slice(inp.firstEdge).map(logs => logs.map(x => (x.ops.length ? [x.ops] : [])))
            const made = engine.changeMany(docs, calls, docs.map(logs => logs.map(() => "a")))
            made.status.forEach(per => per.forEach(st => assert.strictEqual(st, 0)))
            assert.deepStrictEqual(made.changes, call.expectedChanges, "changeMany with the plan's ops: the oracle's Changes")
            made.changes.forEach(per => per.forEach(c => { changes += c.length }))
        }
    }
    assert.throws(() => view.replacePlan("", "x", {}), /needle/)
    assert.throws(() => view.replacePlan("a", 7, {}), /replacement/)
    assert.throws(() => view.replacePlan("a", "x".repeat(65535), {}), /replacement/)
    view.free()
    view.free()
    assert.throws(() => view.replacePlan("a", "b", {}), /freed/)
    return { replaced, skipped, changes }
}

if (mode === "mock") {
    const calls = { applyMaterialize: 0, stringsUpload: 0, stringsFree: 0, viewCreate: 0, viewReplacePlan: 0, viewFree: 0 }
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
        viewReplacePlan(ctx, h, pattern, flags, nReplacement) {
            calls.viewReplacePlan++
            assert.strictEqual(h, view)
            assert.strictEqual(strings, null, "the table was freed after the creation: a plan needs none")
            const needle = String.fromCharCode(...pattern)
            const call = inp.calls.find(c => c.needle === needle)
            assert.ok(call && pattern instanceof Uint16Array, "a needle of the test")
            assert.deepStrictEqual([flags, nReplacement], [call.opts.asciiNocase ? 1 : 0, call.replacement.length])
            const m = call.answer
            return { status: Uint32Array.from(m.status), nMatches: Uint32Array.from(m.nMatches), nChosen: Uint32Array.from(m.nChosen), nReplaced: Uint32Array.from(m.nReplaced), chgOff: big(m.chgOff),
                     opOff: big(m.opOff), action: Uint8Array.from(m.action), index: Uint32Array.from(m.index), count: Uint32Array.from(m.count), kernelMs: 0 }
        },
        viewFree(ctx, h) { calls.viewFree++; assert.strictEqual(h, view); view = null },
    }
    const engine = new host.MergeEngine({ addon: mock })
    const out = check(engine, false)
    assert.deepStrictEqual(calls, { applyMaterialize: 1, stringsUpload: 1, stringsFree: 1, viewCreate: 1, viewReplacePlan: inp.calls.length, viewFree: 1 }, "one view for every call, freed once")
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else if (mode === "gpu") {
    const engine = new host.MergeEngine()
    const out = check(engine, true)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else {
    console.error("usage: node tests/node_replace_check.js mock|gpu IN.json")
    process.exit(2)
}
