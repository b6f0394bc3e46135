/*
 * MergeEngine.textView(docs).markRuns / markSnippets / findInMarks (tests/test_node_markruns.py runs it):
 *   node tests/node_markruns_check.js mock IN.json   no GPU: a stand-in addon hands back the answers tests/test_node_markruns.py computed with the CPU emulation
 *                                                    for the batch both encoders produce (IN.values / IN.payload pin that it IS the same batch)
 *   node tests/node_markruns_check.js gpu IN.json    the real addon on the MI355X
 *   IN = {docs: Change[][][], calls: [{kind: "runs" | "snippets" | "find", sel, opts, needle, expected, ids: the C ABI ids the codec must ask with, answers?}]}
 * Every answer equals the expected one, and, with no help from Python: the runs' (unit, length) are those of a plain loop over the default path's spans that joins
 * neighbours carrying the mark (a link: with the same url; a comment: per id), a snippet's text holds the run's text at matchUnit and its spans join to it, and
 * (on the GPU) every hit of findInMarks is a hit of the same view's findText; one view serves every call and is freed once.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const mode = process.argv[2]
const inp = JSON.parse(fs.readFileSync(process.argv[3], "utf8"))
const MARKS = ["strong", "em", "comment", "link"]
let current = null /* the call in flight: the stand-in answers it */

/* [unit, length, key] of the runs of `sel` in a FormatSpanWithText[]: a plain loop */
function runsOfSpans(spans, sel) {
    const keysOf = marks => {
        if (sel.type === "comment") return (marks.comment || []).map(c => c.id).filter(id => sel.id === undefined || id === sel.id)
        const m = marks[sel.type]
        if (!m || m.active === false) return []
        if (sel.type === "link") return sel.url === undefined || m.url === sel.url ? [m.url] : []
        return [true]
    }
    const out = [], open = new Map()
    let unit = 0
    for (const s of spans.concat([{ text: "", marks: {} }])) {
        const keys = keysOf(s.marks)
        for (const [k, run] of open) if (!keys.includes(k)) { run[1] = unit - run[0]; open.delete(k) }
        for (const k of keys) if (!open.has(k)) { const run = [unit, 0, k]; open.set(k, run); out.push(run) }
        unit += s.text.length
    }
    return out
}
const byUnit = (a, b) => a[0] - b[0] || a[1] - b[1] || String(a[2]).localeCompare(String(b[2]))

function check(engine, twins) {
    const plain = engine.applyChanges(inp.docs)
    const view = engine.textView(inp.docs)
    let runs = 0, snippets = 0, hits = 0
    for (const call of inp.calls) {
        current = call
        const what = call.kind + " " + JSON.stringify(call.sel) + " " + JSON.stringify(call.opts)
        const got = call.kind === "runs" ? view.markRuns(call.sel, call.opts) : call.kind === "snippets" ? view.markSnippets(call.sel, call.opts) : view.findInMarks(call.needle, call.sel, call.opts)
        assert.deepStrictEqual(got, call.expected, what + ": against the plain loop over the oracle's spans")
        const every = twins && call.kind === "find" ? view.findText(call.needle, { ignoreAsciiCase: call.opts.ignoreAsciiCase }) : null
        let log = 0
        inp.docs.forEach((logs, d) => logs.forEach((_, r) => {
            const g = got[d][r], text = plain[d][r].map(s => s.text).join("")
            if (call.kind === "find") {
                if (every) {
                    const all = every[d][r].hits.map(h => JSON.stringify(h))
                    g.hits.forEach(h => assert.ok(all.includes(JSON.stringify(h)), what + ": a contained hit is a hit of findText"))
                    assert.ok(g.count <= every[d][r].count)
                }
                hits += g.hits.length
            } else {
                const want = runsOfSpans(plain[d][r], call.sel)
                assert.strictEqual(g.count, want.length, what + " doc " + d + " replica " + r + ": the number of runs")
                const list = call.kind === "runs" ? g.runs : g.snippets
                const key = x => (call.sel.type === "link" ? x.url : call.sel.type === "comment" ? x.id : true)
                if (call.opts.maxRuns === undefined) assert.deepStrictEqual(list.map(x => [x.unit, x.length, key(x)]).sort(byUnit), want.slice().sort(byUnit), what + ": units of the runs")
                list.forEach(x => {
                    assert.strictEqual(x.log, log)
                    assert.ok(x.start < x.end)
                    if (call.kind === "snippets") {
                        assert.strictEqual(x.text.substr(x.matchUnit, x.length), text.substr(x.unit, x.length), what + ": the run's text stands at matchUnit")
                        assert.strictEqual(x.spans.map(s => s.text).join(""), x.text, what + ": the spans join to the snippet")
                        snippets++
                    } else runs++
                })
            }
            log++
        }))
    }
    current = null
    assert.throws(() => view.markRuns({ type: "bold" }), /sel\.type/)
    assert.throws(() => view.markRuns(undefined), /sel\.type/)
    assert.throws(() => view.markRuns({ type: "link", url: 7 }), /sel\.url/)
    assert.throws(() => view.markSnippets({ type: "strong" }, { before: -1 }), /before/)
    assert.throws(() => view.markRuns({ type: "strong" }, { maxRuns: 2 ** 32 }), /maxRuns/)
    assert.throws(() => view.findInMarks("a", { type: "comment" }), /sel\.id/)
    assert.throws(() => view.findInMarks("", { type: "strong" }), /needle/)
    view.free()
    view.free()
    assert.throws(() => view.markRuns({ type: "strong" }), /freed/)
    return { runs, snippets, hits }
}

if (mode === "mock") {
    const sameBatch = batch => {
        assert.deepStrictEqual(batch.values, inp.values, "the batch is the one the emulation merged")
        assert.deepStrictEqual(Array.from(batch.payload), inp.payload)
    }
    const big = a => BigUint64Array.from(a, BigInt)
    const u32 = a => Uint32Array.from(a)
    const rows = () => ({
        logs: u32(inp.result.logs), values: u32(inp.result.values), spans: u32(inp.result.spans), cintervals: u32(inp.result.cintervals),
        valueOff: big(inp.result.valueOff), spanOff: big(inp.result.spanOff), cintOff: big(inp.result.cintOff),
    })
    const asked = new Map() /* call -> the ids it was asked with */
    const answer = (kind, h, type, id) => {
        assert.strictEqual(h, view)
        assert.strictEqual(strings, null, "the table was freed after the creation: a query needs none")
        assert.ok(current && current.kind === kind && type === MARKS.indexOf(current.sel.type), "the selector's mark type")
        assert.ok(current.ids.includes(id), "an id the codec's tables give: " + id)
        if (!asked.has(current)) asked.set(current, [])
        assert.ok(!asked.get(current).includes(id), "one device call per distinct id")
        asked.get(current).push(id)
        return current.answers[String(id)]
    }
    const runsOf = m => ({ status: u32(m.status), nRuns: u32(m.nRuns), runOff: big(m.runOff), runStart: u32(m.runStart), runEnd: u32(m.runEnd), runId: u32(m.runId), runUnit: u32(m.runUnit),
                           runLen: u32(m.runLen), kernelMs: 0 })
    let strings = null, view = null
    const mock = {
        open() {}, create() { return {} }, destroy() {},
        applyMaterialize(ctx, batch) { sameBatch(batch); return rows() },
        stringsUpload() { assert.strictEqual(strings, null); strings = { table: true }; return strings },
        stringsFree(ctx, h) { assert.strictEqual(h, strings); strings = null },
        viewCreate(ctx, batch, s) {
            sameBatch(batch)
            assert.strictEqual(s, strings, "the table is resident while the view is made")
            assert.strictEqual(view, null, "one view")
            view = { view: true }
            return Object.assign(rows(), { handle: view })
        },
        viewMarkRuns(ctx, h, type, id, cap) {
            const m = answer("runs", h, type, id)
            assert.strictEqual(cap, current.opts.maxRuns === undefined ? 0xFFFFFFFF : current.opts.maxRuns)
            return runsOf(m)
        },
        viewMarkSnippets(ctx, h, type, id, cap, before, after) {
            const m = answer("snippets", h, type, id)
            assert.deepStrictEqual([cap, before, after], [current.opts.maxRuns === undefined ? 0xFFFFFFFF : current.opts.maxRuns, current.opts.before || 0, current.opts.after || 0])
            return Object.assign(runsOf(m), { sliceStatus: u32(m.status), elemStart: u32(m.elemStart), elemEnd: u32(m.elemEnd), unitOff: big(m.unitOff), sspanOff: big(m.sspanOff),
                                              sliceText: Uint16Array.from(m.text), sspans: u32(m.sspans), sspanUnit: u32(m.sspanUnit), matchUnit: u32(m.matchUnit) })
        },
        viewFindInMarks(ctx, h, pattern, flags, type, id, maxHits) {
            const m = answer("find", h, type, id)
            assert.ok(pattern instanceof Uint16Array && String.fromCharCode(...pattern) === current.needle)
            assert.deepStrictEqual([flags, maxHits], [current.opts.ignoreAsciiCase ? 1 : 0, current.opts.maxHits === undefined ? 0xFFFFFFFF : current.opts.maxHits])
            return { status: u32(m.status), nMatches: u32(m.nMatches), hitOff: big(m.hitOff), hitUnit: u32(m.hitUnit), hitStart: u32(m.hitStart), hitEnd: u32(m.hitEnd), kernelMs: 0 }
        },
        viewFree(ctx, h) { assert.strictEqual(h, view); view = null },
    }
    const engine = new host.MergeEngine({ addon: mock })
    const out = check(engine, false)
    for (const call of inp.calls) assert.deepStrictEqual((asked.get(call) || []).slice().sort((a, b) => a - b), call.ids, "the ids asked for: " + JSON.stringify(call.sel))
    assert.strictEqual(view, null, "freed once")
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else if (mode === "gpu") {
    const engine = new host.MergeEngine()
    const out = check(engine, true)
    engine.close()
    console.log(JSON.stringify(Object.assign({ ok: true }, out)))
} else {
    console.error("usage: node tests/node_markruns_check.js mock|gpu IN.json")
    process.exit(2)
}
