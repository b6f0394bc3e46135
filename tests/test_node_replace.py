"""textView.replacePlan of MergeEngine (peritext_amd/node): tests/node_replace_check.js against a stand-in addon on the CPU — the plans it hands back are the CPU
emulation's (tests/test_emu_replace.py) for the very batch both encoders produce — and through the real addon on the MI355X.  In both, every replacePlan answer
must deep-equal the expectation built here by tests/replace_cases.py's sources (the oracle's text searched by a plain loop, a sequential greedy choice, Python
prefix sums, the ops written out in descending order), and the driver applies the ops to the default path's text with no help from Python.  On the GPU
changeMany with the plan's ops returns the oracle's Changes.  The documents: the 46 reference known-answer documents and the chain, blocked, multi-unit,
empty-string and position documents of the replace cases."""
import json
import os
import subprocess

import pytest

import helpers as H
import replace_cases as RC
import test_emu_replace as ER
import test_emu_text as ET
import text_cases as TC
from peritext_amd import wire

DRIVER = os.path.join(H.ROOT, "tests", "node_replace_check.js")
ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")
EDGE_DOCS = ("chain%d" % (RC.S + 1), "abab", "run_over_edge", "blocked", "multi_inside", "multi_end_inside", "multi_start_inside", "multi_one", "multi_two", "empties", "positions", "case")
# (needle, replacement, opts): a frequent letter deleted; folding with a longer replacement; overlap chains; matches inside and across multi-unit values
CALLS = [("e", "", {}), ("t", "<T>", {"asciiNocase": True}), ("aa", "b", {}), ("aba", "xy", {}), ("ab", "Z", {}), ("abcd", "", {})]


def documents():
    """(suite over all documents, docs, the index of the first edge document)"""
    cases = H.load_kat()
    docs = [[r["log"] for r in c["replicas"]] for c in cases]
    want = [TC.want_of_spans(c.get("expected", r["spans"])) for c in cases for r in c["replicas"]]
    edges, names = RC.edge_suite()
    first_edge = len(docs)
    for name in EDGE_DOCS:
        docs.append([wire.decode_changes(edges.batch, names[name])])
        want.append(edges.want[names[name]])
    batch = wire.encode_docs(docs)
    return TC.Suite("node_replace", batch, list(batch.values), want, []), docs, first_edge


def payload_of(with_answers):
    suite, docs, first_edge = documents()
    batch, n = suite.batch, suite.batch.n_logs
    c = ET.compact(batch, H.emu_merge(batch, admission=True), 0, n)
    view = ER.EmuReplaceView(suite, 0, n, 0) if with_answers else None
    calls, replaced = [], 0
    for needle, replacement, opts in CALLS:
        ask = RC.Ask("node_replace", needle, tuple(replacement), nocase=bool(opts.get("asciiNocase")))
        expected, log = [], 0
        for logs in docs:
            per = []
            for _ in logs:
                w = RC.expect(suite, c, 0, log, ask)
                per.append({"log": log, "status": w["status"], "nMatches": w["n_matches"], "nChosen": w["n_chosen"], "nReplaced": w["n_replaced"], "ops": w["ops"]})
                replaced += w["n_replaced"]
                log += 1
            expected.append(per)
        edit_calls = [[[x["ops"]] if x["ops"] else [] for x in per] for per in expected[first_edge:]]
        call = {"needle": needle, "replacement": replacement, "opts": opts, "expected": expected}
        if view is not None:
            p = view.replace_plan(ask, n)
            RC.check_plan(suite, c, p, 0, n, n, ask, RC.ids_of(suite, ask)[0])
            ints = lambda a: [int(x) for x in a]  # noqa: E731
            call["answer"] = {"status": ints(p.status), "nMatches": ints(p.n_matches), "nChosen": ints(p.n_chosen), "nReplaced": ints(p.n_replaced), "chgOff": ints(p.ops.chg_off),
                              "opOff": ints(p.ops.op_off), "action": ints(p.ops.action), "index": ints(p.ops.index), "count": ints(p.ops.count)}
        else:  # the GPU leg: the oracle's change() of the expected ops on the edge documents (one replica each, actor "a")
            flat = H.oracle_change(docs[first_edge:], [x for per in edit_calls for x in per], ["a"] * (len(docs) - first_edge))
            it = iter(flat)
            call["expectedChanges"] = [[[next(it)] if x else [] for x in per] for per in edit_calls]
        calls.append(call)
    one_unit, log = [], 0  # replicas whose every element is ONE code unit: there the driver applies the ops to text.split("") itself
    for logs in docs:
        one_unit.append([all(len(TC.u16(suite.table[int(i)])) == 1 for i in c.values[int(c.value_off[log + r]) : int(c.value_off[log + r + 1])]) for r in range(len(logs))])
        log += len(logs)
    out = {"docs": docs, "firstEdge": first_edge, "oneUnit": one_unit, "calls": calls}
    if view is not None:
        view.close()
        ints = lambda a: [int(x) for x in (a if a.dtype.fields is None else a.view("<u4").reshape(-1))]  # noqa: E731  (structured rows as their u32 words)
        out.update({"values": batch.values, "payload": [int(x) for x in batch.payload],
                    "result": {"logs": ints(c.logs), "values": ints(c.values), "spans": ints(c.spans), "cintervals": ints(c.cintervals), "valueOff": ints(c.value_off), "spanOff": ints(c.span_off),
                               "cintOff": ints(c.cint_off)}})
    return out, replaced, n


def _run(mode, payload, tmp_path, timeout=300):
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    p = subprocess.run([H.NODE, DRIVER, mode, str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@needs_node
@ER.emu
def test_replace_plan_with_the_mock_addon(tmp_path):
    payload, replaced, n = payload_of(True)
    out = _run("mock", payload, tmp_path)
    assert out["ok"] and out["replaced"] == replaced > n and out["skipped"] > 0


@needs_node
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built")
def test_replace_plan_through_the_real_addon(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    payload, replaced, n = payload_of(False)
    out = _run("gpu", payload, tmp_path)
    assert out["ok"] and out["replaced"] == replaced > n and out["skipped"] > 0 and out["changes"] > 0
