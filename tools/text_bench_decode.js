"use strict"
/*
 * The node side of tools/text_bench.py: decodeSpans (one string-table lookup and one concatenation per visible element: today's host join) against
 * decodeSpansText (the log's text built once from the device's UTF-16 buffer, one slice per span) over the SAME downloaded rows of a generated batch.
 *   node tools/text_bench_decode.js <dir with logs.bin values.bin spans.bin cintervals.bin valueOff.bin spanOff.bin cintOff.bin text.bin textOff.bin textStatus.bin spanUnit.bin meta.json>
 * meta = {nLogs, replicas, nComments: per document, reps}.  One warm-up run, then `reps` timed runs of each; medians.  Both must return the same spans (checked on
 * every log once).  Prints one JSON line.
 */
const fs = require("fs")
const path = require("path")
const assert = require("assert")
const host = require(path.join(__dirname, "..", "peritext_amd", "node"))

const dir = process.argv[2]
const meta = JSON.parse(fs.readFileSync(path.join(dir, "meta.json"), "utf8"))
const load = (name, T) => {
    const b = fs.readFileSync(path.join(dir, name + ".bin"))
    const ab = b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)
    return new T(ab)
}
const res = {
    logs: load("logs", Uint32Array), values: load("values", Uint32Array), spans: load("spans", Uint32Array), cintervals: load("cintervals", Uint32Array),
    valueOff: load("valueOff", BigUint64Array), spanOff: load("spanOff", BigUint64Array), cintOff: load("cintOff", BigUint64Array),
    text: load("text", Uint16Array), textOff: load("textOff", BigUint64Array), textStatus: load("textStatus", Uint32Array), spanUnit: load("spanUnit", Uint32Array),
}
/* the fixed tables of a generated batch (include/peritext_hip.h ptx_generate) */
const batch = {
    logOff: new BigUint64Array(meta.nLogs + 1),
    values: Array.from({ length: 128 }, (_, i) => String.fromCharCode(i)),
    urls: Array.from({ length: 26 }, (_, i) => String.fromCharCode(65 + i) + ".com"),
    logDoc: Array.from({ length: meta.nLogs }, (_, l) => Math.floor(l / meta.replicas)),
    docComments: meta.nComments.map(n => Array.from({ length: n }, (_, k) => "comment-" + k).sort()),
}
const median = a => a.slice().sort((x, y) => x - y)[a.length >> 1]
const timed = fn => {
    fn()
    const runs = []
    for (let r = 0; r < meta.reps; r++) {
        const t0 = process.hrtime.bigint()
        fn()
        runs.push(Number(process.hrtime.bigint() - t0) / 1e6)
    }
    return runs
}
let spans = 0, chars = 0
for (let l = 0; l < meta.nLogs; l++) {
    const a = host.decodeSpans(batch, res, l), b = host.decodeSpansText(batch, res, l)
    assert.deepStrictEqual(b, a, "log " + l)
    spans += a.length
    for (const s of a) chars += s.text.length
}
let sink = 0
const join = timed(() => { for (let l = 0; l < meta.nLogs; l++) sink += host.decodeSpans(batch, res, l).length })
const slice = timed(() => { for (let l = 0; l < meta.nLogs; l++) sink += host.decodeSpansText(batch, res, l).length })
console.log(JSON.stringify({ logs: meta.nLogs, spans, chars, decode_spans_join_ms: +median(join).toFixed(3), decode_spans_join_ms_runs: join.map(x => +x.toFixed(3)),
    decode_spans_text_slice_ms: +median(slice).toFixed(3), decode_spans_text_slice_ms_runs: slice.map(x => +x.toFixed(3)), host: "node " + process.version + ", one thread", sink: sink > 0 }))
