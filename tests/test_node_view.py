"""MergeEngine.textView (peritext_amd/node): tests/node_view_check.js against a stand-in addon on the CPU — the answers it hands back are the CPU emulation's of the
view (tests/test_emu_view.py) for the very batch both encoders produce — and through the real addon on the MI355X.  In both, every findSnippets answer must equal
the expectation built here by tests/view_cases.py's sources (the oracle's text searched by a plain loop, Python-integer windows, the oracle's spans cut by a plain
loop), and the driver checks it again with indexOf and slice over the default path's joined span texts.  The documents: the 46 reference known-answer documents
and the span, multi-unit, empty-string and split-pair documents of the slice cases."""
import json
import os
import subprocess

import pytest

import find_cases as FC
import helpers as H
import slice_cases as SC
import test_emu_text as ET
import test_emu_view as EV
import test_node_slices as NS
import view_cases as VC

DRIVER = os.path.join(H.ROOT, "tests", "node_view_check.js")
ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")
needs_emu = pytest.mark.skipif(not os.path.exists(EV.EMU_VIEW_LIB) or not os.path.exists(ET.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_view.so not built (run __graft_entry__.build())")
# (needle, opts): a frequent letter with context on both sides; folding, a cap and a window that saturates at both ends; a needle inside and across multi-unit values
CALLS = [("e", {"before": 1, "after": 1}), ("T", {"ignoreAsciiCase": True, "maxHits": 2, "before": 0xFFFFFFFF, "after": 0xFFFFFFFF}), ("lo, w", {"before": 1, "after": 0}), ("dy", {"before": 2})]


def payload_of(with_answers):
    suite, docs, _ = NS.documents()
    batch, n = suite.batch, suite.batch.n_logs
    res = H.emu_merge(batch, admission=True)
    c = ET.compact(batch, res, 0, n)
    view = EV.EmuView(suite, 0, n, 0) if with_answers else None
    calls, total = [], 0
    for needle, opts in CALLS:
        q = FC.Query(needle, nocase=bool(opts.get("ignoreAsciiCase")), cap=opts.get("maxHits", FC.ALL))
        before, after = opts.get("before", 0), opts.get("after", 0)
        expected, log = [], 0
        for logs in docs:
            per = []
            for _ in logs:
                st, count, listed = FC.expect(suite, c, 0, log, q)
                lv = SC.LogView(suite, c, 0, log)
                snippets = []
                for u, s, e in listed:
                    a, b, units, _, spans = lv.cut(*VC.window(s, e, before, after))
                    snippets.append({"log": log, "hitStart": s, "hitEnd": e, "text": SC.text_of(units), "matchUnit": u - lv.pre[a], "spans": spans})
                per.append({"status": st, "count": count, "snippets": snippets})
                total += len(snippets)
                log += 1
            expected.append(per)
        call = {"needle": needle, "opts": opts, "expected": expected}
        if view is not None:
            m = view.snippets(q, before, after)
            VC.check_snippets(suite, c, m, 0, n, q, before, after)
            ints = lambda a: [int(x) for x in (a if a.dtype.fields is None else a.view("<u4").reshape(-1))]  # noqa: E731  (structured rows as their u32 words)
            call["answer"] = {"status": ints(m.status), "nMatches": ints(m.n_matches), "hitOff": ints(m.slice_off), "hitUnit": ints(m.hit_unit), "hitStart": ints(m.hit_start),
                              "hitEnd": ints(m.hit_end), "elemStart": ints(m.elem_start), "elemEnd": ints(m.elem_end), "unitOff": ints(m.unit_off), "sspanOff": ints(m.sspan_off),
                              "text": ints(m.text), "sspans": ints(m.sspans), "sspanUnit": ints(m.sspan_unit), "matchUnit": ints(m.match_unit)}
        calls.append(call)
    out = {"docs": docs, "calls": calls}
    if view is not None:
        view.close()
        ints = lambda a: [int(x) for x in (a if a.dtype.fields is None else a.view("<u4").reshape(-1))]  # noqa: E731
        out.update({"values": batch.values, "payload": [int(x) for x in batch.payload],
                    "result": {"logs": ints(c.logs), "values": ints(c.values), "spans": ints(c.spans), "cintervals": ints(c.cintervals), "valueOff": ints(c.value_off), "spanOff": ints(c.span_off),
                               "cintOff": ints(c.cint_off)}})
    return out, total, n


def _run(mode, payload, tmp_path, timeout=300):
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    p = subprocess.run([H.NODE, DRIVER, mode, str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@needs_node
@needs_emu
def test_text_view_with_the_mock_addon(tmp_path):
    payload, total, n = payload_of(True)
    out = _run("mock", payload, tmp_path)
    assert out["ok"] and out["snippets"] == total > n and out["rows"] >= total


@needs_node
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built")
def test_text_view_through_the_real_addon(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    payload, total, n = payload_of(False)
    out = _run("gpu", payload, tmp_path)
    assert out["ok"] and out["snippets"] == total > n and out["rows"] >= total
