"""MergeEngine.textSlices (peritext_amd/node): tests/node_slice_check.js against a stand-in addon on the CPU — the slices it hands back are the CPU emulation's for
the very batch both encoders produce — and through the real addon on the MI355X.  In both, every range must equal the oracle's spans cut to it by
tests/slice_cases.py (a plain loop; element boundaries from the value ids of the emulation's merge, which this change leaves alone), and the range that covers a
whole replica must return the default path's spans.  The documents: the 46 reference known-answer documents — a range per span, per comment interval and for the
whole document — and the span, multi-unit, empty-string and split-pair documents of the slice cases with their own ranges."""
import json
import os
import subprocess

import pytest

import helpers as H
import slice_cases as SC
import test_emu_slices as ES
import test_emu_text as ET
import text_cases as TC
from peritext_amd import wire

DRIVER = os.path.join(H.ROOT, "tests", "node_slice_check.js")
ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")
needs_emu = pytest.mark.skipif(not os.path.exists(ES.EMU_SLICE_LIB) or not os.path.exists(ET.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_slice.so not built (run __graft_entry__.build())")
EDGE_DOCS = ("spans", "multi", "empties", "astral_split")


def documents():
    """(suite over all documents, docs, the edge documents' own ranges by log)"""
    cases = H.load_kat()
    docs = [[r["log"] for r in c["replicas"]] for c in cases]
    want = [TC.want_of_spans(c.get("expected", r["spans"])) for c in cases for r in c["replicas"]]
    edges, names = SC.edge_suite()
    plan, _ = SC.edge_plan()
    own = {}
    for name in EDGE_DOCS:
        log = names[name]
        docs.append([wire.decode_changes(edges.batch, log)])
        own[len(want)] = plan[name]
        want.append(edges.want[log])
    batch = wire.encode_docs(docs)
    return TC.Suite("node_slices", batch, list(batch.values), want, []), docs, own


def payload_of(suite, docs, own, with_slices):
    batch = suite.batch
    res = H.emu_merge(batch, admission=True)
    n = batch.n_logs
    c = ET.compact(batch, res, 0, n)
    plan = SC.plan_kat(c, n)
    for log, extra in own.items():
        plan[log] = list(extra) + [(0, SC.ALL)]
    ranges, expected, whole, log = [], [], [], 0
    for logs in docs:
        rr, ee, ww = [], [], []
        for _ in logs:
            view = SC.LogView(suite, c, 0, log)
            rr.append([{"startIndex": s, "endIndex": e} for s, e in plan[log]])
            row = []
            for s, e in plan[log]:
                a, b, _, _, spans = view.cut(s, e)
                row.append({"status": 0, "startIndex": a, "endIndex": b, "spans": spans})
            ee.append(row)
            ww.append(len(plan[log]) - 1)
            log += 1
        ranges.append(rr), expected.append(ee), whole.append(ww)
    out = {"docs": docs, "ranges": ranges, "expected": expected, "whole": whole}
    if with_slices:
        rc, text = ET.emu_text(batch, res, suite.table, 0, n)
        assert rc == 0 and not text.status.any()
        off, start, end = SC.arrays_of(plan)
        rc, m = ES.emu_slices(batch, res, suite.table, text, 0, n, (off, start, end))
        assert rc == 0
        SC.check_range(suite, c, m, 0, n, plan)
        ints = lambda a: [int(x) for x in (a if a.dtype.fields is None else a.view("<u4").reshape(-1))]  # noqa: E731  (structured rows as their u32 words)
        out.update({"values": batch.values, "payload": [int(x) for x in batch.payload],
                    "result": {"logs": ints(c.logs), "values": ints(c.values), "spans": ints(c.spans), "cintervals": ints(c.cintervals), "valueOff": ints(c.value_off), "spanOff": ints(c.span_off),
                               "cintOff": ints(c.cint_off)},
                    "slices": {"sliceOff": ints(off), "sliceStart": ints(start), "sliceEnd": ints(end), "status": ints(m.status), "elemStart": ints(m.elem_start), "elemEnd": ints(m.elem_end),
                               "unitOff": ints(m.unit_off), "sspanOff": ints(m.sspan_off), "text": ints(m.text), "sspans": ints(m.sspans), "sspanUnit": ints(m.sspan_unit)}})
    return out, sum(len(p) for p in plan)


def _run(mode, payload, tmp_path, timeout=300):
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    p = subprocess.run([H.NODE, DRIVER, mode, str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@needs_node
@needs_emu
def test_text_slices_with_the_mock_addon(tmp_path):
    suite, docs, own = documents()
    payload, n_ranges = payload_of(suite, docs, own, True)
    out = _run("mock", payload, tmp_path)
    assert out["ok"] and out["checked"] == n_ranges > suite.batch.n_logs and out["rows"] > suite.batch.n_logs


@needs_node
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built")
def test_text_slices_through_the_real_addon(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    suite, docs, own = documents()
    payload, n_ranges = payload_of(suite, docs, own, False)
    out = _run("gpu", payload, tmp_path)
    assert out["ok"] and out["checked"] == n_ranges > suite.batch.n_logs and out["rows"] > suite.batch.n_logs
