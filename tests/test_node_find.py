"""MergeEngine.findText (peritext_amd/node): tests/node_find_check.js against a stand-in addon on the CPU — the matches it hands back are the CPU emulation's for
the very batch both encoders produce — and through the real addon on the MI355X.  In both, a replica's count and hit units must equal indexOf repeated over the
default path's joined span texts, and the element ranges the values tests/find_cases.py computes (a plain loop over the expected text; element boundaries from
the value ids of the emulation's merge, which this change leaves alone).  The documents: the 46 reference known-answer documents and the multi-unit, empty-string,
astral and case documents of the find cases."""
import json
import os
import subprocess

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import test_emu_find as EF
import test_emu_text as ET
import text_cases as TC
from peritext_amd import wire

DRIVER = os.path.join(H.ROOT, "tests", "node_find_check.js")
ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")
needs_emu = pytest.mark.skipif(not os.path.exists(EF.EMU_FIND_LIB) or not os.path.exists(ET.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_find.so not built (run __graft_entry__.build())")
QUERIES = [("e", {}), ("TH", {"ignoreAsciiCase": True}), ("\ud83d", {}), ("world", {"maxHits": 1}), ("a", {"maxHits": 0}), ("he", {"maxHits": 2, "ignoreAsciiCase": True})]


def documents():
    """(suite over all documents, docs)"""
    cases = H.load_kat()
    docs = [[r["log"] for r in c["replicas"]] for c in cases]
    want = [TC.want_of_spans(c.get("expected", r["spans"])) for c in cases for r in c["replicas"]]
    edges, names = FC.edge_suite()
    for name in ("multi", "empties", "astral_one_value", "astral_split", "case"):
        log = names[name]
        docs.append([wire.decode_changes(edges.batch, log)])
        want.append(edges.want[log])
    batch = wire.encode_docs(docs)
    return TC.Suite("node_find", batch, list(batch.values), want, []), docs


def payload_of(suite, docs, with_matches):
    batch = suite.batch
    res = H.emu_merge(batch, admission=True)
    n = batch.n_logs
    c = ET.compact(batch, res, 0, n)
    queries = []
    for needle, opts in QUERIES:
        q = FC.Query(needle, nocase=bool(opts.get("ignoreAsciiCase")), cap=opts.get("maxHits", FC.ALL))
        expected, log = [], 0
        for logs in docs:
            row = []
            for _ in logs:
                st, count, listed = FC.expect(suite, c, 0, log, q)
                row.append({"status": st, "count": count, "hits": [{"unit": u, "startIndex": s, "endIndex": e} for u, s, e in listed]})
                log += 1
            expected.append(row)
        entry = {"needle": needle, "opts": opts, "expected": expected}
        if with_matches:
            rc, text = ET.emu_text(batch, res, suite.table, 0, n)
            assert rc == 0 and not text.status.any()
            rc, m = EF.emu_find(batch, res, suite.table, text, 0, n, q)
            assert rc == 0
            ints = lambda a: [int(x) for x in a]  # noqa: E731
            entry["matches"] = {"status": ints(m.status), "nMatches": ints(m.n_matches), "hitOff": ints(m.hit_off), "hitUnit": ints(m.hit_unit), "hitStart": ints(m.hit_start), "hitEnd": ints(m.hit_end)}
        queries.append(entry)
    out = {"docs": docs, "queries": queries}
    if with_matches:
        ints = lambda a: [int(x) for x in (a if a.dtype == np.uint64 else a.view("<u4").reshape(-1))]  # noqa: E731  (structured rows as their u32 words)
        out.update({"values": batch.values, "payload": [int(x) for x in batch.payload],
                    "result": {"logs": ints(c.logs), "values": ints(c.values), "spans": ints(c.spans), "cintervals": ints(c.cintervals), "valueOff": ints(c.value_off), "spanOff": ints(c.span_off),
                               "cintOff": ints(c.cint_off)}})
    return out


def _run(mode, payload, tmp_path, timeout=300):
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    p = subprocess.run([H.NODE, DRIVER, mode, str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@needs_node
@needs_emu
def test_find_text_with_the_mock_addon(tmp_path):
    suite, docs = documents()
    out = _run("mock", payload_of(suite, docs, True), tmp_path)
    assert out["ok"] and out["checked"] == suite.batch.n_logs * len(QUERIES) and out["hits"] > suite.batch.n_logs


@needs_node
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built")
def test_find_text_through_the_real_addon(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    suite, docs = documents()
    out = _run("gpu", payload_of(suite, docs, False), tmp_path)
    assert out["ok"] and out["checked"] == suite.batch.n_logs * len(QUERIES) and out["hits"] > suite.batch.n_logs
