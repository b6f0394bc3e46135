"""MergeEngine.applyChanges / documentsAt with { text: "device" } (peritext_amd/node): tests/node_text_check.js against a stand-in addon on the CPU — the rows
and the text it hands back are the CPU emulation's for the very batch both encoders produce — and through the real addon on the MI355X.  The documents: the
46 reference known-answer documents (expected = the reference-held literal, else the oracle's spans), the astral character as one value, the surrogate pair
split over two elements (expected = the hand-written literal of tests/text_cases.py) and the alternating-bold document."""
import json
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import test_emu_text as ET
import text_cases as TC
from peritext_amd import wire

DRIVER = os.path.join(H.ROOT, "tests", "node_text_check.js")
ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")


def documents():
    """(docs, expected spans per doc and replica)"""
    cases = H.load_kat()
    docs = [[r["log"] for r in c["replicas"]] for c in cases]
    expected = [[c.get("expected", r["spans"]) for r in c["replicas"]] for c in cases]
    names, edge = TC.edge_docs()
    want = dict(zip(names, TC.edge_suite().want))
    for name in ("astral_one_value", "alternating_bold", "empty_strings"):
        docs.append(edge[names.index(name)])
        expected.append([want[name].spans])
    docs.append([H.mini_doc([], first_text=TC.SPLIT_PAIR_VALUES)])
    expected.append([[{"text": TC.SPLIT_PAIR_TEXT, "marks": {}}]])
    return docs, expected


def _run(mode, payload, tmp_path, timeout=300):
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    p = subprocess.run([H.NODE, DRIVER, mode, str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@needs_node
@pytest.mark.skipif(not os.path.exists(ET.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_text.so not built (run __graft_entry__.build())")
def test_device_text_equals_the_default_path_with_the_mock_addon(tmp_path):
    docs, expected = documents()
    batch = wire.encode_docs(docs)
    res = H.emu_merge(batch, admission=True)
    rc, text = ET.emu_text(batch, res, batch.values, 0, batch.n_logs)
    assert rc == 0 and not text.status.any()
    c = ET.compact(batch, res, 0, batch.n_logs)
    ints = lambda a: [int(x) for x in (a if a.dtype == np.uint64 else a.view("<u4").reshape(-1))]  # noqa: E731  (structured rows as their u32 words)
    payload = {
        "docs": docs, "expected": expected, "values": batch.values, "payload": [int(x) for x in batch.payload],
        "result": {"logs": ints(c.logs), "values": ints(c.values), "spans": ints(c.spans), "cintervals": ints(c.cintervals),
                   "valueOff": ints(c.value_off), "spanOff": ints(c.span_off), "cintOff": ints(c.cint_off)},
        "text": {"text": [int(x) for x in text.text], "textOff": [int(x) for x in text.text_off], "status": [int(x) for x in text.status], "spanUnit": [int(x) for x in text.span_unit]},
    }
    out = _run("mock", payload, tmp_path)
    assert out["ok"] and out["checked"] == batch.n_logs


@needs_node
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built")
def test_device_text_through_the_real_addon(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    docs, expected = documents()
    out = _run("gpu", {"docs": docs, "expected": expected}, tmp_path)
    assert out["ok"] and out["checked"] == sum(len(d) for d in docs) and out["versions"] > out["checked"]
