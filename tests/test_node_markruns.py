"""MergeEngine.textView(docs).markRuns / markSnippets / findInMarks (peritext_amd/node): tests/node_markruns_check.js against a stand-in addon on the CPU — the
answers it hands back are the CPU emulation's (tests/test_emu_markruns.py) for the very batch both encoders produce — and through the real addon on the MI355X.  In
both, every answer must equal the expectation built here from tests/markrun_cases.py's sources (a plain loop over the oracle's spans, Python string lengths, the
oracle's spans cut by a plain loop, find_cases' hits filtered by a plain loop), and the driver checks the runs again, with no help from Python, against a loop over
the default path's spans.  The documents: the 46 reference known-answer documents and the link, comment, empty-string, multi-unit and step-edge documents of the
mark-run cases.  A comment id is turned into its rank per document by the codec: the stand-in sees one call per distinct rank."""
import json
import os
import subprocess

import pytest

import find_cases as FC
import helpers as H
import markrun_cases as MC
import slice_cases as SC
import test_emu_markruns as EM
import test_emu_text as ET
import text_cases as TC
from peritext_amd import wire

DRIVER = os.path.join(H.ROOT, "tests", "node_markruns_check.js")
ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")
needs_emu = pytest.mark.skipif(not os.path.exists(EM.EMU_LIB) or not os.path.exists(ET.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_markruns.so not built (run __graft_entry__.build())")
EDGE_DOCS = ["links", "comments", "empties", "fim", "r62_65", "alt", "plain"]
MARK_OF = {"strong": MC.STRONG, "em": MC.EM, "link": MC.LINK, "comment": MC.COMMENT}


def documents():
    cases = H.load_kat()
    docs = [[r["log"] for r in c["replicas"]] for c in cases]
    want = [TC.want_of_spans(c.get("expected", r["spans"])) for c in cases for r in c["replicas"]]
    edges, names = MC.edge_suite()
    for name in EDGE_DOCS:
        docs.append([wire.decode_changes(edges.batch, names[name])])
        want.append(edges.want[names[name]])
    batch = wire.encode_docs(docs)
    return TC.Suite("node_markruns", batch, list(batch.values), want, []), docs


def calls_of(suite):
    batch = suite.batch
    some_comment = next(c[0] for c in batch.doc_comments if c)
    return [
        ("runs", {"type": "strong"}, {}, None),
        ("runs", {"type": "em"}, {"maxRuns": 2}, None),
        ("runs", {"type": "link"}, {}, None),
        ("runs", {"type": "link", "url": "a.com"}, {}, None),
        ("runs", {"type": "link", "url": "nowhere.example"}, {}, None),
        ("runs", {"type": "comment"}, {}, None),
        ("runs", {"type": "comment", "id": "c-A"}, {}, None),
        ("runs", {"type": "comment", "id": "no-such-comment"}, {}, None),
        ("snippets", {"type": "comment"}, {}, None),
        ("snippets", {"type": "comment", "id": some_comment}, {"before": 1, "after": 2}, None),
        ("snippets", {"type": "link"}, {"before": 0xFFFFFFFF, "after": 0xFFFFFFFF, "maxRuns": 1}, None),
        ("snippets", {"type": "strong"}, {"before": 1, "after": 1}, None),
        ("find", {"type": "strong"}, {}, "abc"),
        ("find", {"type": "strong"}, {"maxHits": 2, "ignoreAsciiCase": True}, "E"),
        ("find", {"type": "link"}, {}, "e"),
        ("find", {"type": "comment", "id": "c-B"}, {}, "e"),
    ]


def _ident(batch, log, sel):
    mt = MARK_OF[sel["type"]]
    key = sel.get("url") if mt == MC.LINK else sel.get("id")
    if key is None:
        return MC.ANY
    table = batch.urls if mt == MC.LINK else batch.doc_comments[batch.log_doc[log]]
    return list(table).index(key) if key in table else (len(table) if mt == MC.LINK else 0xFFFFFFFE)  # the codec's "an id nothing has"


def _run_json(batch, log, sel, run):
    s, e, rid, unit, length = run
    out = {"log": log, "start": s, "end": e, "unit": unit, "length": length}
    if sel["type"] == "link":
        out["url"] = batch.urls[rid]
    if sel["type"] == "comment":
        out["id"] = batch.doc_comments[batch.log_doc[log]][rid]
    return out


def payload_of(with_answers):
    suite, docs = documents()
    batch, n = suite.batch, suite.batch.n_logs
    res = H.emu_merge(batch, admission=True)
    c = ET.compact(batch, res, 0, n)
    view = EM.EmuMarkView(suite, 0, n, 0) if with_answers else None
    ints = lambda a: [int(x) for x in (a if a.dtype.fields is None else a.view("<u4").reshape(-1))]  # noqa: E731  (structured rows as their u32 words)
    calls, totals = [], {"runs": 0, "snippets": 0, "find": 0}
    for kind, sel, opts, needle in calls_of(suite):
        mt = MARK_OF[sel["type"]]
        cap = opts.get("maxRuns", MC.ALL)
        before, after = opts.get("before", 0), opts.get("after", 0)
        q = FC.Query(needle, nocase=bool(opts.get("ignoreAsciiCase")), cap=opts.get("maxHits", MC.ALL)) if needle else None
        expected, idents, log = [], set(), 0
        for logs in docs:
            per = []
            for _ in logs:
                ident = _ident(batch, log, sel)
                idents.add(ident)
                lv = SC.LogView(suite, c, 0, log)
                runs = MC.expect_runs(suite, lv, log, mt, ident)
                if kind == "runs":
                    per.append({"status": 0, "count": len(runs), "runs": [_run_json(batch, log, sel, r) for r in runs[:cap]]})
                elif kind == "snippets":
                    snippets = []
                    for r in runs[:cap]:
                        a, b, units, _, spans = lv.cut(*MC.window(r[0], r[1], before, after))
                        snippets.append(dict(_run_json(batch, log, sel, r), text=SC.text_of(units), spans=spans, matchUnit=r[3] - lv.pre[a]))
                    per.append({"status": 0, "count": len(runs), "snippets": snippets})
                else:
                    kept = MC.expect_contained(suite, c, 0, log, q, runs)
                    per.append({"status": 0, "count": len(kept), "hits": [{"unit": u, "startIndex": s, "endIndex": e} for u, s, e in kept[: q.cap]]})
                totals[kind] += len(per[-1][{"runs": "runs", "snippets": "snippets", "find": "hits"}[kind]])
                log += 1
            expected.append(per)
        call = {"kind": kind, "sel": sel, "opts": opts, "needle": needle, "expected": expected, "ids": sorted(idents)}
        if view is not None:
            call["answers"] = {}
            for ident in sorted(idents):
                if kind == "find":
                    m = view.find_in_marks(q, mt, ident)
                    call["answers"][str(ident)] = {"status": ints(m.status), "nMatches": ints(m.n_matches), "hitOff": ints(m.hit_off), "hitUnit": ints(m.hit_unit), "hitStart": ints(m.hit_start),
                                                   "hitEnd": ints(m.hit_end)}
                    continue
                m = view.mark_snippets(mt, ident, cap, before, after) if kind == "snippets" else view.mark_runs(mt, ident, cap)
                a = {"status": ints(m.status), "nRuns": ints(m.n_runs), "runOff": ints(m.run_off), "runStart": ints(m.run_start), "runEnd": ints(m.run_end), "runId": ints(m.run_id),
                     "runUnit": ints(m.run_unit), "runLen": ints(m.run_len)}
                if kind == "snippets":
                    a.update({"elemStart": ints(m.elem_start), "elemEnd": ints(m.elem_end), "unitOff": ints(m.unit_off), "sspanOff": ints(m.sspan_off), "text": ints(m.text),
                              "sspans": ints(m.sspans), "sspanUnit": ints(m.sspan_unit), "matchUnit": ints(m.match_unit)})
                call["answers"][str(ident)] = a
        calls.append(call)
    out = {"docs": docs, "calls": calls}
    if view is not None:
        view.close()
        out.update({"values": batch.values, "payload": [int(x) for x in batch.payload],
                    "result": {"logs": ints(c.logs), "values": ints(c.values), "spans": ints(c.spans), "cintervals": ints(c.cintervals), "valueOff": ints(c.value_off), "spanOff": ints(c.span_off),
                               "cintOff": ints(c.cint_off)}})
    assert all(v > 0 for v in totals.values()), totals
    return out, totals


def _run(mode, payload, tmp_path, timeout=300):
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    p = subprocess.run([H.NODE, DRIVER, mode, str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@needs_node
@needs_emu
def test_mark_queries_with_the_mock_addon(tmp_path):
    payload, totals = payload_of(True)
    out = _run("mock", payload, tmp_path)
    assert out["ok"] and out["runs"] == totals["runs"] and out["snippets"] == totals["snippets"] and out["hits"] == totals["find"]


@needs_node
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built")
def test_mark_queries_through_the_real_addon(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    payload, totals = payload_of(False)
    out = _run("gpu", payload, tmp_path)
    assert out["ok"] and out["runs"] == totals["runs"] and out["snippets"] == totals["snippets"] and out["hits"] == totals["find"]
